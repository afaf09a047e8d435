"""-m gpu: the two checkpoint-to-samples entry points (test_text_to_image_control_lora.py, test_dreambooth_lora.py) end to end on
the small random model at resolution 64: a two-step run of the matching training script writes `checkpoint-2`, the script loads
it, writes the final weights in both formats and `samples/<name>/{0,1}.png` with 4 DPM-Solver++ steps on the one-launch sampler
step."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_control_lora_checkpoint_to_weights_and_strips(tmp_path):
    import numpy as np
    from PIL import Image
    from safetensors.torch import load_file
    from oracle import cases
    import test_text_to_image_control_lora as S
    import train_text_to_image_control_lora as T
    cfg = tmp_path / "small.json"
    cfg.write_text(json.dumps({k: (list(v) if isinstance(v, tuple) else v) for k, v in cases.SMALL_CLORA_V1.items()}))
    out = tmp_path / "run-clora"
    common = ["--pretrained_model_name_or_path", "random:small", "--dataset_name", "synthetic:fill50k", "--control_lora_config", str(cfg),
              "--output_dir", str(out), "--resolution", "64", "--train_batch_size", "2", "--max_train_samples", "16", "--seed", "3",
              "--mixed_precision", "fp16"]
    assert T.main(common + ["--max_train_steps", "2", "--checkpointing_steps", "2", "--learning_rate", "1e-2"]) == 2
    assert os.path.isdir(out / "checkpoint-2")
    for f in ("config.json", "diffusion_pytorch_model.bin", "diffusion_pytorch_model.safetensors"):
        os.remove(out / f)                                             # what the training run left: the script must write its own
    sample_args = ["--num_validation_images", "2", "--num_inference_steps", "4", "--validation_prompt", "red circle with blue background",
                   "--samples_dir", str(tmp_path / "samples")]
    with pytest.raises(ValueError, match="does not exist"):
        S.main(common + sample_args + ["--resume_from_checkpoint", "checkpoint-7"])
    assert not (out / "config.json").exists(), "a missing checkpoint must stop the script before it writes anything"
    paths = S.main(common + sample_args + ["--resume_from_checkpoint", "latest"])
    assert paths == [str(tmp_path / "samples" / "run-clora" / f"{i}.png") for i in range(2)]
    for f in ("config.json", "diffusion_pytorch_model.bin", "diffusion_pytorch_model.safetensors"):
        assert (out / f).exists(), f
    strips = [np.asarray(Image.open(p)) for p in paths]
    assert all(s.shape == (64, 3 * 64, 3) for s in strips), [s.shape for s in strips]
    assert not np.array_equal(strips[0], strips[1])                    # another data set item and another draw of the one generator
    ds = T.build_dataset(S.parse_args(common + sample_args), tokenizer=None)
    for i, s in enumerate(strips):                                     # [target | guide | image] of the unshuffled items 0, 1
        ex = ds[i]
        for j, key in enumerate(("pixel_values", "guide_values")):
            want = ((ex[key] + 1.0) * 127.5).permute(1, 2, 0).numpy().clip(0, 255).astype(np.uint8)
            assert np.array_equal(s[:, j * 64:(j + 1) * 64], want), (i, key)
        assert s[:, 128:].std() > 0
    # the saved weights are the checkpoint's, in both formats
    ckpt = torch.load(out / "checkpoint-2" / "diffusion_pytorch_model.bin", map_location="cpu", weights_only=True)
    safe = load_file(str(out / "diffusion_pytorch_model.safetensors"))
    binf = torch.load(out / "diffusion_pytorch_model.bin", map_location="cpu", weights_only=True)
    assert set(ckpt) == set(safe) == set(binf)
    for k, v in ckpt.items():
        assert torch.equal(safe[k], v) and torch.equal(binf[k], v), k
    # the host step implementation writes the same files
    again = S.main(common + sample_args + ["--resume_from_checkpoint", "checkpoint-2", "--sampler_step", "host"])
    host = [np.asarray(Image.open(p)).astype(np.int32) for p in again]
    for h, s in zip(host, strips):
        assert np.array_equal(h[:, :128], s[:, :128])
        print("SAMPLER_SCRIPT control-lora: mean |device - host| of the sampled panel (uint8 levels):", float(np.abs(h[:, 128:] - s[:, 128:]).mean()))


def test_dreambooth_checkpoint_to_weights_and_samples(tmp_path):
    import numpy as np
    from PIL import Image
    from safetensors.torch import load_file
    import test_dreambooth_lora as S
    import train_dreambooth_lora as T
    inst = tmp_path / "instance"
    os.makedirs(inst)
    rng = np.random.default_rng(0)
    for i in range(2):
        Image.fromarray(rng.integers(0, 255, (80, 72, 3), dtype=np.uint8)).save(inst / f"{i}.png")
    out = tmp_path / "run-lora"
    common = ["--pretrained_model_name_or_path", "random:small", "--instance_data_dir", str(inst), "--instance_prompt", "a photo of sks dog",
              "--resolution", "64", "--train_batch_size", "2", "--seed", "3", "--output_dir", str(out)]
    assert T.main(common + ["--max_train_steps", "2", "--checkpointing_steps", "2", "--learning_rate", "1e-2"]) == 2
    assert os.path.isdir(out / "checkpoint-2")
    for f in ("pytorch_lora_weights.bin", "pytorch_lora_weights.safetensors"):
        os.remove(out / f)
    sample_args = ["--num_validation_images", "2", "--num_inference_steps", "4", "--validation_prompt", "a photo of sks dog",
                   "--samples_dir", str(tmp_path / "samples")]
    paths = S.main(common + sample_args + ["--resume_from_checkpoint", "latest"])
    assert paths == [str(tmp_path / "samples" / "run-lora" / f"{i}.png") for i in range(2)]
    imgs = [np.asarray(Image.open(p)) for p in paths]
    assert all(im.shape == (64, 64, 3) for im in imgs) and not np.array_equal(imgs[0], imgs[1])
    ckpt = load_file(str(out / "checkpoint-2" / "pytorch_lora_weights.safetensors"))
    safe = load_file(str(out / "pytorch_lora_weights.safetensors"))
    binf = torch.load(out / "pytorch_lora_weights.bin", map_location="cpu", weights_only=True)
    assert set(ckpt) == set(safe) == set(binf)
    for k, v in ckpt.items():
        assert torch.equal(safe[k], v) and torch.equal(binf[k], v), k
    assert any(float(v.abs().max()) > 0 for k, v in safe.items() if k.endswith("to_q_lora.up.weight"))     # trained, not the zero init
    # a missing checkpoint is logged, not an error: the freshly initialised adapters (zero `up`) are written
    fresh = tmp_path / "fresh"
    S.main([a if a != str(out) else str(fresh) for a in common] + ["--num_validation_images", "0", "--validation_prompt", "a photo of sks dog",
                                                                   "--samples_dir", str(tmp_path / "samples"), "--resume_from_checkpoint", "latest"])
    zero = load_file(str(fresh / "pytorch_lora_weights.safetensors"))
    assert all(float(v.abs().max()) == 0 for k, v in zero.items() if k.endswith("lora.up.weight"))
    assert os.listdir(tmp_path / "samples" / "fresh") == []
