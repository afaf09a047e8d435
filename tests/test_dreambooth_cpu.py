"""CPU tests of the DreamBooth-LoRA entry point's host side: the reference's flags, the diffusers LoRA file writer, the data set."""
import os

import numpy as np
import pytest
import torch

import train_dreambooth_lora as T
from controllora_amd import data, loading, text

REFERENCE_DEFAULTS = dict(
    pretrained_model_name_or_path="x", revision=None, tokenizer_name=None, instance_data_dir="i", class_data_dir=None, instance_prompt="p",
    class_prompt=None, validation_prompt=None, num_validation_images=4, validation_epochs=50, with_prior_preservation=False,
    prior_loss_weight=1.0, num_class_images=100, output_dir="lora-dreambooth-model", seed=None, resolution=512, center_crop=False,
    train_batch_size=4, sample_batch_size=4, num_train_epochs=1, max_train_steps=None, checkpointing_steps=500,
    checkpoints_total_limit=None, resume_from_checkpoint=None, gradient_accumulation_steps=1, gradient_checkpointing=False,
    learning_rate=5e-4, scale_lr=False, lr_scheduler="constant", lr_warmup_steps=500, lr_num_cycles=1, lr_power=1.0,
    dataloader_num_workers=0, use_8bit_adam=False, adam_beta1=0.9, adam_beta2=0.999, adam_weight_decay=1e-2, adam_epsilon=1e-08,
    max_grad_norm=1.0, push_to_hub=False, hub_token=None, hub_model_id=None, logging_dir="logs", allow_tf32=False, report_to="tensorboard",
    mixed_precision=None, prior_generation_precision=None, local_rank=-1, enable_xformers_memory_efficient_attention=False, lora_rank=4)
REQUIRED = ["--pretrained_model_name_or_path", "x", "--instance_data_dir", "i", "--instance_prompt", "p"]


def test_all_reference_flags_are_accepted_with_reference_defaults(monkeypatch):
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    assert len(REFERENCE_DEFAULTS) == 50
    a = T.parse_args(REQUIRED)
    for k, v in REFERENCE_DEFAULTS.items():
        assert getattr(a, k) == v and type(getattr(a, k)) is type(v), (k, getattr(a, k), v)
    b = T.parse_args(REQUIRED + ["--with_prior_preservation", "--class_data_dir", "c", "--class_prompt", "q", "--prior_loss_weight", "0.5",
                                 "--lr_num_cycles", "3", "--lr_power", "2.0", "--checkpoints_total_limit", "2", "--center_crop",
                                 "--prior_generation_precision", "fp16", "--tokenizer_name", "t", "--sample_batch_size", "2"])
    assert b.with_prior_preservation and b.prior_loss_weight == 0.5 and b.lr_num_cycles == 3 and b.checkpoints_total_limit == 2 and b.center_crop
    with pytest.raises(SystemExit):
        T.parse_args(REQUIRED[:4])                           # --instance_prompt is required


def test_the_two_argument_errors():
    with pytest.raises(ValueError, match="data directory for class images"):
        T.parse_args(REQUIRED + ["--with_prior_preservation", "--class_prompt", "q"])
    with pytest.raises(ValueError, match="prompt for class images"):
        T.parse_args(REQUIRED + ["--with_prior_preservation", "--class_data_dir", "c"])
    with pytest.warns(UserWarning, match="class_data_dir"):
        T.parse_args(REQUIRED + ["--class_data_dir", "c"])


def test_lr_num_cycles_and_power_reach_the_schedule():
    f1, f3 = data.lr_lambda("cosine_with_restarts", 0, 90), data.lr_lambda("cosine_with_restarts", 0, 90, restarts=3)
    assert f1(30) == pytest.approx(0.75) and f3(30) == pytest.approx(1.0) and f3(15) == pytest.approx(0.5)
    assert data.lr_lambda("polynomial", 0, 100, power=2.0)(50) == pytest.approx(0.25, abs=1e-6)


def _small_unet():
    from controllora_amd import unet as U
    return U.UNet2DConditionModel(**loading.SMALL_UNET)


def test_lora_file_round_trip_through_both_file_types(tmp_path):
    unet = _small_unet()
    procs = T.build_lora_processors(unet, 6, "cpu")
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in procs.values():
            for q in p.parameters():
                q.copy_(torch.randn(q.shape, generator=g))
    unet.set_attn_processor(procs)
    parts = [f"to_{s}_lora.{d}.weight" for s in ("q", "k", "v", "out") for d in ("down", "up")]
    want = {f"{n}.{part}" for n in unet.attn_processors for part in parts}
    assert all(n.endswith(".processor") for n in unet.attn_processors) and len(want) == 8 * len(procs)
    paths = [loading.save_lora_attn_procs(unet, str(tmp_path / "a")), loading.save_lora_attn_procs(procs, str(tmp_path / "b"), safe_serialization=True),
             unet.save_attn_procs(str(tmp_path / "c"), weights_name="pytorch_lora_weights.bin", save_function=torch.save),
             unet.save_attn_procs(str(tmp_path / "d"), weights_name="pytorch_lora_weights.safetensors", safe_serialization=True)]
    assert [os.path.basename(p) for p in paths] == ["pytorch_lora_weights.bin", "pytorch_lora_weights.safetensors"] * 2
    assert all(os.path.basename(p) in loading.LORA_FILE_NAMES for p in paths)
    for path in paths:
        sd = loading._read_lora_file(os.path.dirname(path))
        assert set(sd) == want and all(v.dtype == torch.float32 for v in sd.values())
        loaded = loading.load_lora_attn_procs(unet, os.path.dirname(path))
        assert list(loaded) == list(procs)
        for n, p in procs.items():
            assert loaded[n].rank == 6
            for k, v in p.state_dict().items():
                assert torch.equal(loaded[n].state_dict()[k], v), (n, k)
    fresh = _small_unet()
    fresh.load_attn_procs(str(tmp_path / "d"))
    for n, p in fresh.attn_processors.items():
        assert torch.equal(p.to_out_lora.up.weight, procs[n].to_out_lora.up.weight)
    with pytest.raises(ValueError, match="not a plain LoRA processor"):
        loading.save_lora_attn_procs(_small_unet(), str(tmp_path / "e"))


def _folders(tmp_path, n_inst, n_class, size=(96, 64)):
    from PIL import Image
    rng = np.random.default_rng(0)
    for name, n in (("inst", n_inst), ("cls", n_class)):
        os.makedirs(tmp_path / name)
        for i in range(n):
            Image.fromarray(rng.integers(0, 255, (size[1], size[0], 3), dtype=np.uint8)).save(tmp_path / name / f"{i}.png")
    return str(tmp_path / "inst"), str(tmp_path / "cls")


def test_dataset_length_modulo_indexing_and_collate_order(tmp_path):
    inst, cls = _folders(tmp_path, 2, 5)
    tok = text.HashTokenizer()
    ds = data.DreamBoothDataset(inst, "a photo of sks dog", tok, cls, "a photo of a dog", size=32, center_crop=True)
    assert len(ds) == 5 and len(data.DreamBoothDataset(inst, "p", tok, size=32)) == 2
    assert torch.equal(ds[4]["instance_images"], ds[0]["instance_images"]) and torch.equal(ds[3]["instance_images"], ds[1]["instance_images"])
    assert not torch.equal(ds[0]["instance_images"], ds[1]["instance_images"])
    assert not torch.equal(ds[4]["class_images"], ds[0]["class_images"])
    assert "class_images" not in data.DreamBoothDataset(inst, "p", tok, size=32)[0]
    ex = [ds[0], ds[1], ds[2]]
    b = data.dreambooth_collate(ex, True)
    assert b["pixel_values"].shape == (6, 3, 32, 32) and b["pixel_values"].dtype == torch.float32 and b["input_ids"].shape == (6, 77)
    for i in range(3):
        assert torch.equal(b["pixel_values"][i], ex[i]["instance_images"]) and torch.equal(b["pixel_values"][3 + i], ex[i]["class_images"])
        assert torch.equal(b["input_ids"][i], tok(["a photo of sks dog"])[0]) and torch.equal(b["input_ids"][3 + i], tok(["a photo of a dog"])[0])
    assert data.dreambooth_collate(ex, False)["pixel_values"].shape == (3, 3, 32, 32)
    with pytest.raises(ValueError):
        data.DreamBoothDataset(str(tmp_path / "nothing"), "p", tok)


def test_centre_crop_and_random_crop_on_a_96x64_image(tmp_path):
    from PIL import Image
    inst, _ = _folders(tmp_path, 1, 0)
    tok = text.HashTokenizer()
    img = Image.open(os.path.join(inst, "0.png")).convert("RGB").resize((48, 32), Image.BILINEAR)      # short side 64 -> 32
    full = torch.from_numpy(np.asarray(img, dtype=np.float32) / 255.0).permute(2, 0, 1) * 2.0 - 1.0
    centre = data.DreamBoothDataset(inst, "p", tok, size=32, center_crop=True)[0]["instance_images"]
    assert centre.shape == (3, 32, 32) and float(centre.min()) >= -1.0 and float(centre.max()) <= 1.0
    assert torch.allclose(centre, full[:, :, 8:40], atol=1e-6)                      # (48 - 32) / 2 = 8 columns off each side
    ds = data.DreamBoothDataset(inst, "p", tok, size=32)
    torch.manual_seed(0)
    a = ds[0]["instance_images"]
    torch.manual_seed(0)
    top, left = int(torch.randint(0, 1, (1,))), int(torch.randint(0, 17, (1,)))      # the crop comes from torch's global generator
    assert top == 0 and torch.allclose(a, full[:, :, left:left + 32], atol=1e-6)
    lefts = set()
    for _ in range(8):
        c = ds[0]["instance_images"]
        lefts.update(x for x in range(17) if torch.allclose(c, full[:, :, x:x + 32], atol=1e-6))
    assert len(lefts) > 1


def test_entry_point_refuses_to_run_without_a_gpu(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="MI355X"):
        T.main(REQUIRED + ["--output_dir", str(tmp_path)])


def test_sampling_without_a_guide_needs_a_size():
    from controllora_amd.pipeline import ddim_sample
    e = torch.zeros(1, 7, 64, dtype=torch.float16)
    with pytest.raises(ValueError, match="size"):
        ddim_sample(None, None, None, e, e, steps=1)
    with pytest.raises(ValueError, match="guide"):
        ddim_sample(None, object(), None, e, e, steps=1)
