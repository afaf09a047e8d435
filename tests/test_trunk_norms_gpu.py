"""GPU tests (-m gpu): the norms that read the compensated trunk (CLORA_TRUNK_LO=norms) on the gfx950 library -- the shapes that select
each GroupNorm plan on the device and the (M, C) lists of the LayerNorm tests (tests/trunk_norm_cases.py states the limits)."""
import pytest
import torch

from tests import trunk_norm_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda"


# team: (4, 4096, 320), (4, 1024, 640); one block per slab: (4, 256, 1280); two launches: (3, 1000, 640), (2, 300, 64)
@pytest.mark.parametrize("B,HW,C,G", [(4, 4096, 320, 32), (4, 1024, 640, 32), (4, 256, 1280, 32), (3, 1000, 640, 32), (2, 300, 64, 8)])
def test_groupnorm_reads_hi_plus_lo(B, HW, C, G):
    TC.case_groupnorm_lo(DEV, B, HW, C, G)


def test_groupnorm_reads_hi_plus_lo_with_silu():
    TC.case_groupnorm_lo(DEV, 2, 300, 64, 8, silu=True)


@pytest.mark.parametrize("B,HW,Ca,Cb,G,silu", [(4, 4096, 320, 320, 32, True), (4, 4096, 640, 320, 32, False), (4, 1024, 640, 640, 32, True),
                                               (4, 1024, 1280, 640, 32, False), (4, 256, 1280, 1280, 32, True), (4, 64, 1280, 1280, 32, True),
                                               (1, 300, 64, 32, 8, False)])
def test_groupnorm_concat_reads_hi_plus_lo(B, HW, Ca, Cb, G, silu):
    TC.case_groupnorm_lo_concat(DEV, B, HW, Ca, Cb, G, silu)


def test_groupnorm_lo_rejects_a_deferred_source():
    TC.case_groupnorm_lo_rejects_deferred(DEV, B=4, HW=256, C=1280, Kd=2560, G=32, split=4)


@pytest.mark.parametrize("M,C", [(4096, 320), (1024, 640), (259, 1280), (16384, 320), (4099, 640), (2049, 1280), (1024, 1280), (308, 768)])
def test_layernorm_reads_hi_plus_lo(M, C):
    TC.case_layernorm_lo(DEV, M, C)


def test_blocks_in_norms_mode():
    TC.case_blocks_norms(DEV)


def test_small_unet_modes(monkeypatch):
    unet, _, inp, _ = TC.case_small_unet_modes(DEV, monkeypatch)
    TC.check_infer_is_trunklo_true(unet, inp, DEV, monkeypatch)


def test_ddim_graph_equals_eager_in_norms_mode(monkeypatch):
    """a captured forward replays the `_lo` launches with the remainders that lived in the capture's pool: the same bits as eager"""
    from controllora_amd import kernels as K
    from controllora_amd.pipeline import ddim_sample
    from oracle import cases
    from tests import e2e_cases as E
    monkeypatch.setattr(K, "TRUNK_LO_MODE", "norms")
    inp = cases.seeded_inputs()
    unet, _, clora = E.build_product_case("v1", DEV)
    guide = inp["guide"][:1].to(DEV).half()
    cond, uncond = inp["ehs"][:1].to(DEV).half(), inp["ehs"][1:2].to(DEV).half()
    lat = inp["latents"][:1].to(DEV).half()
    with TC.call_counter() as cc:
        eager = ddim_sample(unet, clora, guide, cond, uncond, steps=3, latents=lat.clone(), graph=False)
    assert cc.lo_calls() > 0
    graphed = ddim_sample(unet, clora, guide, cond, uncond, steps=3, latents=lat.clone(), graph=True)
    torch.cuda.synchronize()
    assert torch.isfinite(eager).all() and torch.equal(eager, graphed)
