"""-m gpu: mixing several ControlLoRAs on the real library -- the control-mix kernel at SD-1.5's q-block shapes, the fused v1 site
at a real width, switches and staleness, a whole small UNet and the sampler under two control models (eager and replayed graph), the
pipeline with lists, and apps/multi_control2image.py end to end."""
import copy
import os
import sys

import pytest
import torch

from controllora_amd import capi, kernels as K, models as M
from tests import multi_control_cases as MC

pytestmark = pytest.mark.gpu
f16 = torch.float16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = dict(B=2, side=16, C=320, heads=8, ctx=768)


# ------------------------------------------------------------------------------------------------ 2. kernel
@pytest.mark.parametrize("Mr,C,ldy,ranks,div", MC.KERNEL_SHAPES)
def test_control_mix_kernel_matches_fp64(Mr, C, ldy, ranks, div):
    MC.check_mix_against_fp64(Mr, C, ldy, ranks, div, dev="cuda")


@pytest.mark.parametrize("Mr,C,ldy,ranks,div", [
    (2 * 4096, 320, 960, (4, 4), 2),                          # the widest-token site's q block: many chunks per block column
    (2 * 1024, 640, 640, (4, 12, 16), 1),                     # a cross-attention q output, the full 32 ranks
])
def test_control_mix_kernel_at_sd15_q_blocks(Mr, C, ldy, ranks, div):
    MC.check_mix_against_fp64(Mr, C, ldy, ranks, div, dev="cuda", many_elements=True)


def test_control_mix_contract_breaches_are_refused():
    MC.check_contract_breaches("cuda")
    y, members, rows_t = MC.mix_inputs(48, 72, 216, (4,), 1, dev="cuda")
    with pytest.raises(capi.CloraError):
        K.control_mix_q(y.cpu(), 72, members, rows_t)         # no CPU fallback


# ------------------------------------------------------------------------------------------------ 3. fused site
@pytest.mark.parametrize("arrangement", MC.ARRANGEMENTS)
def test_fused_site_matches_oracle_chain(arrangement):
    MC.check_fused_site(arrangement, "cuda")


@pytest.mark.parametrize("arrangement", MC.ARRANGEMENTS)
def test_fused_site_matches_oracle_chain_at_a_real_width(arrangement):
    MC.check_fused_site(arrangement, "cuda", **REAL)


# ------------------------------------------------------------------------------------------------ 4. - 6. switches, staleness, broadcast
def _out(s, p_main=None, **kw):
    with torch.no_grad():
        return MC.product_site(s, p_main, **kw)


def _fresh(s):
    p = copy.deepcopy(s["p_main"])
    p.__dict__.pop("_fold", None)
    p.__dict__.pop("_mix", None)
    return p


@pytest.mark.parametrize("self_attn", [True, False])
def test_switches_staleness_and_broadcast(self_attn):
    s = MC.build_site(self_attn, "two_control", "cuda")
    p = s["p_main"]
    base = _out(s)
    for fold_chain in (False, True):                          # the new switch off: today's generic path, bit for bit
        p.fold_chain, p.fold_control_members = fold_chain, False
        assert torch.equal(_out(s), base) and "_fold" not in p.__dict__ and "_mix" not in p.__dict__
    y0 = _out(s, fused=True)
    mix0 = p.__dict__["_mix"]
    assert torch.equal(y0, _out(s)) and p.__dict__["_mix"] is mix0
    MC.inject_member_controls(s, scale_by=-0.5)               # new control states: the output moves as the oracle says
    y1 = _out(s)
    yo = MC.oracle_site(s)
    assert MC.rel(y1, yo) < MC.TOL_Y and MC.rel(y0, yo) > 2 * MC.TOL_Y, (MC.rel(y1, yo), MC.rel(y0, yo))
    with torch.no_grad():                                     # an in-place change of a member's q up matrix
        p.pre_loras[0].to_q_lora.up.weight.mul_(-1.5)
    y2 = _out(s)
    assert not torch.equal(y2, y1) and torch.equal(y2, _out(s, _fresh(s)))
    for what in ("autograd on", "post_add member"):           # blockers: generic, and no fold state appears
        s2 = MC.build_site(self_attn, "control_pre", "cuda", **(dict(member_kw=dict(post_add=True)) if what == "post_add member" else {}))
        grad = what == "autograd on"
        off = MC.product_site(s2, fused=False, grad=grad).detach()
        s2["p_main"].fold_chain = s2["p_main"].fold_control_members = True
        with torch.set_grad_enabled(grad):
            assert s2["p_main"]._fold_blocker() is not None
        assert torch.equal(MC.product_site(s2, grad=grad).detach(), off) and "_mix" not in s2["p_main"].__dict__
    one = MC.build_site(self_attn, "two_control", "cuda", ctrl_batch=1)
    tiled = MC.build_site(self_attn, "two_control", "cuda", ctrl_batch=1)
    tiled["member_ctrl"] = {k: v.repeat(tiled["B"], 1, 1, 1) for k, v in tiled["member_ctrl"].items()}
    MC.inject_member_controls(tiled)
    assert torch.equal(_out(one, fused=True), _out(tiled, fused=True))


# ------------------------------------------------------------------------------------------------ 7. whole small UNet
def test_two_control_unet_matches_oracle_and_adds_one_launch_per_site():
    MC.check_two_control_unet("cuda")


def test_sampler_takes_lists_and_a_list_of_one_is_the_single_call():
    MC.check_sampler_lists("cuda")


def test_two_control_ddim_small_50_steps_fused_generic_and_graph():
    """the settings and limits of test_mixed_folded_ddim_small_50_steps, under two control models"""
    case = MC.two_control_sampler_case("cuda")
    fused = MC.two_control_sample(case, "cuda", fused=True, graph=False)
    replay = MC.two_control_sample(case, "cuda", fused=True, graph=True)
    generic = MC.two_control_sample(case, "cuda", fused=False, graph=False)
    r = dict(fused=MC.rel(fused, case["ref"]), generic=MC.rel(generic, case["ref"]), fp16_oracle_vs_fp32_oracle=case["floor"])
    print("TWO_CONTROL DDIM_LATENT_PARITY small 50 steps", r)
    assert torch.equal(fused, replay), "the replayed graph must equal the eager sampler bit for bit"
    for k in ("fused", "generic"):
        assert r[k] < 5.5e-3 and r[k] < r["fp16_oracle_vs_fp32_oracle"] * 1.1, r


def test_pipeline_takes_lists():
    from controllora_amd.pipeline import ControlLoRAPipeline
    from oracle import cases
    torch.manual_seed(3)
    _, a = MC.seeded_control_pair("v1", "cuda", seed=51)
    _, b = MC.seeded_control_pair("v1", "cuda", seed=52)
    g = torch.Generator().manual_seed(2)
    g1, g2 = (torch.rand(1, 3, 64, 64, generator=g) * 2 - 1 for _ in range(2))
    kw = dict(num_samples=1, ddim_steps=4, scale=5.0, seed=1)
    single = ControlLoRAPipeline.from_pretrained("random:small", a, "cuda")("a red circle", g1, **kw)
    listed = ControlLoRAPipeline.from_pretrained("random:small", [a], "cuda")
    assert torch.equal(listed("a red circle", [g1], **kw), single) and torch.equal(listed("a red circle", g1, **kw), single)
    two = ControlLoRAPipeline.from_pretrained("random:small", [a, b], "cuda")
    img = two("a red circle", [g1, g2], **kw)
    with torch.no_grad():
        assert all(r["folded"] and r["control_members"] == 1 for r in two.control_lora[0].fold_report().values())
    assert img.shape == single.shape == (1, 64, 64, 3) and not torch.equal(img, single)
    with pytest.raises(ValueError, match="guide"):
        two("a red circle", [g1], **kw)


# ------------------------------------------------------------------------------------------------ 8. entry point
def test_multi_control_app_writes_guides_and_images(tmp_path, capsys):
    import numpy as np
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "apps"))
    import multi_control2image as app
    dirs = []
    for i, seed in enumerate((61, 62)):
        _, m = MC.seeded_control_pair("v1", "cpu", seed=seed)
        m.save_pretrained(str(tmp_path / f"clora{i}"))
        dirs.append(str(tmp_path / f"clora{i}"))
    rng = np.random.default_rng(0)
    photo = np.zeros((64, 64, 3), np.uint8)
    photo[16:48, 20:44] = 220
    Image.fromarray(photo).save(tmp_path / "photo.png")
    Image.fromarray(rng.integers(0, 255, (64, 64, 3), dtype=np.uint8)).save(tmp_path / "pose.png")
    common = ["--base", "random:sd15-small", "--control_lora", dirs[0], "--guide", "canny", "--control_lora", dirs[1], "--guide",
              str(tmp_path / "pose.png"), "--input", str(tmp_path / "photo.png"), "--prompt", "red circle", "--image_resolution", "64",
              "--sample_steps", "4", "--num_samples", "2", "--seed", "7"]
    sites = 32
    assert app.main(common + ["--out", str(tmp_path / "fused.png")]) == sites
    assert f"{sites} of {sites} sites fused" in capsys.readouterr().out
    assert app.main(common + ["--no_fold", "--out", str(tmp_path / "generic.png")]) == 0
    assert f"0 of {sites} sites fused" in capsys.readouterr().out
    a, b = np.asarray(Image.open(tmp_path / "fused.png")), np.asarray(Image.open(tmp_path / "generic.png"))
    assert a.shape == b.shape == (64, 64 * 4, 3), a.shape                 # [guide_0 | guide_1 | image | image]
    assert np.array_equal(a[:, :128], b[:, :128]) and a[:, :64].min() == 0, "the left part is the guides"
    assert np.abs(a[:, 128:].astype(int) - b[:, 128:].astype(int)).mean() < 8, "fused and generic images agree"
    with pytest.raises(SystemExit):
        app.main(common[:6] + common[8:])                                # a control model without its guide
