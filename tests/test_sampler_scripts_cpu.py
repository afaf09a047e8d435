"""CPU: the argument handling of the two checkpoint-to-samples entry points (test_text_to_image_control_lora.py,
test_dreambooth_lora.py) -- the training scripts' flags plus their own, how `--resume_from_checkpoint` is resolved inside
`--output_dir`, where the samples go, and that neither runs without a GPU."""
import os

import pytest
import torch

import test_dreambooth_lora as SD
import test_text_to_image_control_lora as SC
import train_dreambooth_lora as TD
import train_text_to_image_control_lora as TC

CLORA = ["--pretrained_model_name_or_path", "random:small", "--dataset_name", "synthetic:fill50k", "--control_lora_config", "c.json"]
DREAM = ["--pretrained_model_name_or_path", "random:small", "--instance_data_dir", "dog", "--instance_prompt", "a photo of sks dog"]


def test_flags_are_the_training_scripts_plus_three():
    a, t = SC.parse_args(CLORA), TC.parse_args(CLORA)
    assert {k: v for k, v in vars(a).items() if k in vars(t)} == vars(t)
    assert set(vars(a)) - set(vars(t)) == {"num_inference_steps", "sampler_step", "samples_dir"}
    assert (a.num_inference_steps, a.sampler_step, a.samples_dir) == (30, "device", "samples")
    d, t = SD.parse_args(DREAM), TD.parse_args(DREAM)
    assert {k: v for k, v in vars(d).items() if k in vars(t)} == vars(t)
    assert set(vars(d)) - set(vars(t)) == {"num_inference_steps", "sampler_step", "samples_dir"}
    assert (d.num_inference_steps, d.sampler_step, d.samples_dir) == (25, "device", "samples")
    b = SC.parse_args(["--sampler_step", "host"] + CLORA + ["--num_inference_steps", "12", "--resolution", "64", "--num_validation_images", "2"])
    assert (b.sampler_step, b.num_inference_steps, b.resolution, b.num_validation_images) == ("host", 12, 64, 2)
    with pytest.raises(SystemExit):
        SC.parse_args(CLORA + ["--sampler_step", "gpu"])
    with pytest.raises(SystemExit):
        SD.parse_args(DREAM + ["--no_such_flag", "1"])
    with pytest.raises(ValueError):                          # the training script's own check (reference :322-324) still runs
        SC.parse_args(["--pretrained_model_name_or_path", "x", "--control_lora_config", "c.json"])


@pytest.mark.parametrize("mod,base", [(SC, CLORA), (SD, DREAM)])
def test_checkpoint_resolution(mod, base, tmp_path):
    out = tmp_path / "run"
    args = lambda *extra: mod.parse_args(base + ["--output_dir", str(out)] + list(extra))

    def expect_none(a):
        if mod is SC:                                        # the ControlLoRA script: a named but missing checkpoint is an error
            with pytest.raises(ValueError, match="does not exist"):
                mod.resolve_checkpoint(a)
        else:                                                # the DreamBooth script logs it and goes on
            assert mod.resolve_checkpoint(a) is None
    assert mod.resolve_checkpoint(args()) is None            # no flag: nothing to load, in both
    expect_none(args("--resume_from_checkpoint", "latest"))  # no output directory yet
    os.makedirs(out / "checkpoint-10")
    os.makedirs(out / "checkpoint-9")
    os.makedirs(out / "logs")
    (out / "checkpoint-77").write_text("a file, not a checkpoint")
    expect_none(args("--resume_from_checkpoint", "checkpoint-77"))
    os.remove(out / "checkpoint-77")
    assert mod.resolve_checkpoint(args("--resume_from_checkpoint", "latest")) == str(out / "checkpoint-10")       # numeric, not lexical
    assert mod.resolve_checkpoint(args("--resume_from_checkpoint", "checkpoint-9")) == str(out / "checkpoint-9")
    assert mod.resolve_checkpoint(args("--resume_from_checkpoint", "/elsewhere/run/checkpoint-9/")) == str(out / "checkpoint-9")  # basename only
    expect_none(args("--resume_from_checkpoint", "checkpoint-3"))


@pytest.mark.parametrize("mod,base", [(SC, CLORA), (SD, DREAM)])
def test_samples_go_under_the_basename_of_the_output_dir(mod, base, tmp_path):
    a = mod.parse_args(base + ["--output_dir", "/some/where/my-run/"])
    assert mod.samples_dir(a) == os.path.join("samples", "my-run")
    b = mod.parse_args(base + ["--output_dir", str(tmp_path / "x"), "--samples_dir", str(tmp_path / "s")])
    assert mod.samples_dir(b) == str(tmp_path / "s" / "x")


@pytest.mark.parametrize("mod,base", [(SC, CLORA), (SD, DREAM)])
def test_scripts_refuse_to_run_without_a_gpu(mod, base, tmp_path):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="MI355X"):
        mod.main(base + ["--output_dir", str(tmp_path / "run")])
    assert not (tmp_path / "run").exists()
