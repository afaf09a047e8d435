"""GPU: the VAE past 8,192 latent tokens (768 x 768 images) and at non-square sizes, on the wide flash forward kernel."""
import os

import pytest
import torch

from tests import vae_wide_cases as VW

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("batch,th,tw", [(1, 96, 96), (2, 24, 40)], ids=["768x768", "2x192x320"])
def test_vae_attention_block_matches_oracle(batch, th, tw):
    """VaeAttention(512, 32) against oracle.vae_ref.AttentionBlock in fp64 on the device: the 9,216 tokens of a 768 x 768 image
    (more than the materialised scores can take), and a non-square batch of two in one launch (both paths measured)"""
    VW.check_attention_block("cuda", batch, th, tw)


@pytest.mark.parametrize("flash", [None, True], ids=["default_path", "flash"])
def test_vae_sd15_widths_non_square_matches_oracle(flash):
    """the SD-1.5 VAE at its real widths, 128 x 192, batch 2 (384 tokens in the mid-block attention): on the default attention path
    and with the flash path pinned"""
    from controllora_amd import vae as V
    VW.check_vae_rect("cuda", 128, 192, batch=2, cfg=V.SD15_VAE, tol=6e-3, flash=flash)


def test_pipeline_768_random_sd15():
    """the largest size of the reference apps' image_resolution slider end to end: one sample, 2 DPM-Solver++ steps at 96 x 96
    latents, then the VAE decode over 9,216 tokens; the same image for the same seed"""
    from controllora_amd import models as M
    from controllora_amd.pipeline import ControlLoRAPipeline
    torch.manual_seed(0)
    clora = M.ControlLoRA.from_config(os.path.join(ROOT, "configs", "fill50k.json"))
    pipe = ControlLoRAPipeline.from_pretrained("random:sd15", clora, "cuda")
    guide = torch.rand(1, 3, 768, 768) * 2 - 1
    a = pipe("red circle", guide, num_samples=1, ddim_steps=2, scale=7.5, seed=5, sampler="dpm")
    b = pipe("red circle", guide, num_samples=1, ddim_steps=2, scale=7.5, seed=5, sampler="dpm")
    assert a.shape == (1, 768, 768, 3) and a.dtype == torch.uint8
    assert int(a.max()) > int(a.min()) and torch.equal(a, b)
