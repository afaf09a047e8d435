"""-m gpu: chained version-2 ControlLoRAs on the real library -- the control-chain kernel (clora_control_chain_f16) against fp64, the
fused v2 site against the oracle chain, the recorded reference outputs through the fused path, blockers and stale jobs, a captured UNet
forward, the sampler under two v2 control models (eager and replayed graph), and apps/multi_control2image.py end to end."""
import os
import sys

import pytest
import torch

from controllora_amd import capi, kernels as K
from tests import multi_control_cases as MC
from tests import multi_control_v2_cases as V2

pytestmark = pytest.mark.gpu
f16 = torch.float16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. kernel
@pytest.mark.parametrize("Mr,C,ranks,div", V2.KERNEL_SHAPES)
def test_control_chain_kernel_matches_fp64(Mr, C, ranks, div):
    V2.check_chain_against_fp64(Mr, C, ranks, div, dev="cuda")


def test_control_chain_kernel_in_place_and_with_pitches_and_offsets():
    V2.check_chain_against_fp64(75, 72, (4, 12, 16), 3, dev="cuda", in_place=True)
    V2.check_chain_against_fp64(128, 320, (4, 4), 1, dev="cuda", padded=True)
    V2.check_chain_against_fp64(3 * 128 + 21, 72, (8, 8), 3, dev="cuda", in_place=True, padded=True)


@pytest.mark.parametrize("Mr,C,ranks,div", [
    (32 * 4096, 320, (4, 4), 32),               # the widest-token site of a 16-image sampler: four rows per lane group
    (8 * 4096, 640, (4, 4), 8),                 # two rows per lane group in each rank class
    (8 * 4096, 640, (4, 8), 8),
    (8 * 4096, 640, (16, 16), 8),
    (16, 1288, (4, 4), 1),                      # the full-wave row layout
    (8, 2560, (4, 8), 1),
])
def test_control_chain_kernel_every_launch_variant(Mr, C, ranks, div):
    V2.check_chain_against_fp64(Mr, C, ranks, div, dev="cuda")


def test_control_chain_kernel_ranks_off_the_four_rank_batches():
    """the kernel walks the stacked ranks four at a time: totals that end inside a batch, members that straddle one"""
    for ranks, div in (((3, 5), 1), ((1, 2), 2), ((5,), 1), ((7, 6, 1), 1), ((16, 9), 2)):
        V2.check_chain_against_fp64(40, 72, ranks, div, dev="cuda")


def test_control_chain_contract_breaches_are_refused():
    V2.check_contract_breaches("cuda")
    H, members, G, rows_t = V2.chain_inputs(48, 72, (4,), 1, dev="cuda")
    with pytest.raises(capi.CloraError):
        K.control_chain(H.cpu(), torch.empty_like(H).cpu(), members, None, 0.7, rows_t)      # no CPU fallback


# ------------------------------------------------------------------------------------------------ 2. + 3. fused site
@pytest.mark.parametrize("arrangement", V2.ARRANGEMENTS)
def test_fused_v2_site_matches_oracle_chain(arrangement):
    V2.check_fused_site(arrangement, "cuda")


# ------------------------------------------------------------------------------------------------ 4. records
def test_fused_path_reproduces_the_v2_records():
    records = MC.load_records()
    names = [n for n in sorted(records) if n.split(":")[0] in V2.V2_RECORD_CASES]
    assert len(names) == 8, names
    for name in names:
        y, ya, _ = V2.replay_record_fused(name, records[name], "cuda")
        e = V2.rel(y, ya)
        print(f"MULTI_CONTROL_V2_RECORD {name}: fused path {e:.3e} (limit {V2.TOL_Y})")
        assert e < V2.TOL_Y, (name, e)


# ------------------------------------------------------------------------------------------------ 5. blockers, staleness, capture
@pytest.mark.parametrize("what", V2.BLOCKERS)
def test_ineligible_v2_chains_report_a_blocker_and_run_generic(what):
    for self_attn in (True, False):
        V2.check_blocker(what, self_attn, "cuda")


@pytest.mark.parametrize("self_attn", [True, False])
def test_a_stale_chain_job_is_never_served(self_attn):
    V2.check_staleness(self_attn, "cuda")


def test_captured_unet_forward_replays_the_eager_result_and_a_new_guide_in_a_capture_raises():
    inp = MC.small_inputs()
    g = torch.Generator().manual_seed(9)
    guides = [inp["guide"], torch.rand(inp["guide"].shape, generator=g) * 2 - 1]
    _, _, unet, cl = MC.two_control_small_pair("cuda", fold=True, case="v2")
    MC.forward(unet, cl, inp, guides, "cuda")                  # folds and builds the jobs: not part of a captured step
    x, ehs = inp["latents"].half().cuda(), inp["ehs"].half().cuda()
    t = torch.full((1,), 501, device="cuda", dtype=torch.long)  # the timestep lives on the device, as in pipeline.ddim_sample
    with torch.no_grad():
        assert all(r["folded"] for r in cl[0].fold_report().values())
        eager = unet(x, t, ehs).sample.clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = unet(x, t, ehs).sample
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), "the replayed graph must equal the eager forward bit for bit"
        cl[1](-guides[1][:1].half().cuda())                     # a new guide for the member: every site's job is stale
        other = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="inside a graph capture"):
            with torch.cuda.graph(other):
                unet(x, t, ehs)
        torch.cuda.synchronize()
        assert not torch.equal(unet(x, t, ehs).sample, eager)   # outside a capture the jobs are rebuilt


# ------------------------------------------------------------------------------------------------ 6. whole small UNet
def test_two_v2_control_unet_matches_oracle_with_two_chain_launches_per_site():
    V2.check_two_control_unet("cuda")


def test_two_v2_control_ddim_small_50_steps_fused_generic_and_graph():
    """the settings and limits of test_two_control_ddim_small_50_steps_fused_generic_and_graph, under two v2 control models"""
    case = V2.two_control_sampler_case("cuda")
    fused = MC.two_control_sample(case, "cuda", fused=True, graph=False)
    replay = MC.two_control_sample(case, "cuda", fused=True, graph=True)
    generic = MC.two_control_sample(case, "cuda", fused=False, graph=False)
    r = dict(fused=MC.rel(fused, case["ref"]), generic=MC.rel(generic, case["ref"]), fp16_oracle_vs_fp32_oracle=case["floor"])
    print("TWO_CONTROL_V2 DDIM_LATENT_PARITY small 50 steps", r)
    assert torch.equal(fused, replay), "the replayed graph must equal the eager sampler bit for bit"
    for k in ("fused", "generic"):
        assert r[k] < 5.5e-3 and r[k] < r["fp16_oracle_vs_fp32_oracle"] * 1.1, r


def test_multi_control_app_on_two_v2_models(tmp_path, capsys):
    import numpy as np
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "apps"))
    import multi_control2image as app
    dirs = []
    for i, seed in enumerate((61, 62)):
        _, m = MC.seeded_control_pair("v2", "cpu", seed=seed)
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
    assert np.array_equal(a[:, :128], b[:, :128]), "the left part is the guides"
    assert np.abs(a[:, 128:].astype(int) - b[:, 128:].astype(int)).mean() < 8, "fused and generic images agree"
