"""CPU tests of the DreamBooth-LoRA path on the emulated kernels: the per-sample-weighted MSE launch and one train step of the
plain-LoRA trainer (prior preservation against the oracle with autograd, the plain step against the reference's golden)."""
import pytest

from tests import dreambooth_cases as D
from tests.emu_fixture import use_emulator


@pytest.fixture(autouse=True)
def _emu():
    with use_emulator():
        yield


@pytest.mark.parametrize("B,n", D.KERNEL_SHAPES)
def test_weighted_mse_with_unit_weights_is_the_plain_mse(B, n):
    D.check_unit_weights_equal_plain_mse(B, n, "cpu")


@pytest.mark.parametrize("B,n", D.KERNEL_SHAPES)
def test_weighted_mse_mixed_weights_against_fp64(B, n):
    D.check_mixed_weights_against_fp64(B, n, "cpu")


def test_weighted_mse_argument_errors():
    D.check_argument_errors("cpu")


def test_prior_preservation_step_matches_oracle_autograd():
    D.check_prior_preservation_step("cpu")


def test_plain_step_through_the_lora_trainer_matches_reference_golden(golden_dir):
    D.check_plain_step_against_golden("cpu", golden_dir)


def test_lora_trainer_checkpoint_round_trip(tmp_path):
    """save_state writes trainer_state.safetensors and the diffusers LoRA file; load_state restores the flat state bit for bit; the
    accelerate layout is not read"""
    import os
    import torch
    from controllora_amd import loading
    a = D.make_trainer("cpu")
    g = torch.Generator().manual_seed(5)
    a.flat.grad += torch.randn(a.flat.numel, generator=g) * 128.0
    a.optimizer_step()
    a.save_state(str(tmp_path / "checkpoint-1"))
    assert sorted(os.listdir(tmp_path / "checkpoint-1")) == ["pytorch_lora_weights.safetensors", "trainer_state.safetensors"]
    b = D.make_trainer("cpu")
    assert not torch.equal(a.flat.data, b.flat.data)
    b.load_state(str(tmp_path / "checkpoint-1"))
    assert torch.equal(a.flat.data, b.flat.data) and torch.equal(a.flat.exp_avg_sq, b.flat.exp_avg_sq) and b.global_step == 1
    procs = loading.load_lora_attn_procs(b.unet, str(tmp_path / "checkpoint-1"))
    for name, p in b.unet.attn_processors.items():
        for k, v in p.state_dict().items():
            assert torch.equal(procs[name].state_dict()[k], v), (name, k)
    os.makedirs(tmp_path / "accelerate")
    with pytest.raises(FileNotFoundError):
        b.load_state(str(tmp_path / "accelerate"))


def test_loss_scalars_before_a_step_and_with_a_wrong_size():
    tr = D.make_trainer("cpu")
    with pytest.raises(RuntimeError, match="last step"):
        tr.loss()
    with pytest.raises(RuntimeError, match="last step"):
        tr.loss_parts()
    assert tr.sample_sums is None
    pred = tr.forward_backward(*D.step_args("cpu", 4), D.prior_weights("cpu"))
    assert tr.loss(pred.numel()) == tr.loss()
    with pytest.raises(ValueError, match="elements"):
        tr.loss(pred.numel() // 2)


def test_per_sample_sums_of_a_batch_size_are_never_rebound():
    """a captured graph holds the address of the sums it was captured with: a step of another batch size in between gets a buffer
    of its own, and the first one is neither replaced nor written"""
    import torch
    tr = D.make_trainer("cpu")
    args4, w4 = D.step_args("cpu", 4), D.prior_weights("cpu")
    tr.forward_backward(*args4, w4)
    buf4, parts4, loss4 = tr.sample_sums, tr.loss_parts(), tr.loss()
    kept = buf4.clone()
    args2 = tuple(a[:2].contiguous() for a in D.step_args("cpu", 2))
    tr.forward_backward(*args2, torch.tensor([1.0, D.PRIOR_WEIGHT]))
    assert tr.sample_sums.numel() == 2 and tr.sample_sums.data_ptr() != buf4.data_ptr()
    assert tr._sums[4] is buf4 and torch.equal(buf4, kept)
    assert tr.loss_parts() != parts4
    tr.forward_backward(*args4, w4)
    assert tr.sample_sums is buf4 and tr.loss_parts() == parts4 and tr.loss() == loss4
