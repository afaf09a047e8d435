"""CPU (host-emulated kernels): the VAE's mid-block attention on the wide flash forward kernel, non-square images through the small
random pipeline, and the loud limit of the materialised-scores fallback."""
import pytest
import torch

from tests import vae_wide_cases as VW
from tests.emu_fixture import use_emulator


@pytest.fixture(autouse=True)
def _emulated():
    with use_emulator():
        yield


def test_vae_with_a_256_wide_head_matches_oracle():
    """last width 256: the mid-block attention (16 tokens of a 32 x 32 image) runs the wide kernel; a non-square size as well"""
    VW.check_vae_rect("cpu", 32, 32, batch=1, flash=True)
    VW.check_vae_rect("cpu", 32, 48, batch=2, flash=True)
    VW.check_vae_rect("cpu", 32, 48, batch=2, flash=False)   # 24 tokens: the scores path beside it


def test_vae_attention_block_matches_oracle_on_both_paths():
    VW.check_attention_block("cpu", 2, 4, 6, c=256, groups=8)     # the scores path needs a multiple of 8 tokens


def test_pipeline_at_non_square_sizes():
    """the sizes resize_image produces (multiples of 64, H != W): uint8 [1, H, W, 3], the same image for the same seed"""
    from controllora_amd import models as M
    from controllora_amd.pipeline import ControlLoRAPipeline
    from oracle import cases
    torch.manual_seed(0)
    pipe = ControlLoRAPipeline.from_pretrained("random:small", M.ControlLoRA(**cases.SMALL_CLORA_V1), "cpu")
    for h, w in ((64, 128), (192, 64)):
        guide = torch.rand(1, 3, h, w) * 2 - 1
        a = pipe("red circle", guide, num_samples=1, ddim_steps=2, scale=5.0, seed=5, sampler="dpm")
        b = pipe("red circle", guide, num_samples=1, ddim_steps=2, scale=5.0, seed=5, sampler="dpm")
        assert a.shape == (1, h, w, 3) and a.dtype == torch.uint8 and torch.equal(a, b) and int(a.max()) > int(a.min())


def test_scores_fallback_names_both_limits():
    """a head wider than the flash kernels take, over more tokens than the materialised scores take: a ValueError before any launch"""
    from controllora_amd import vae as V
    m = V.VaeAttention(576, 8)                               # weights never read: the check comes first
    with pytest.raises(ValueError, match=r"512.*8192"):
        m(torch.zeros(1, 8200, 576, dtype=torch.float16))
