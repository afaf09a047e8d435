"""-m gpu: folding frozen chained LoRAs into the frozen attention weights on the real library -- the fold kernel at SD-1.5's
shapes, the folded site at a real width, samplers on whole UNets with every site mixed identically in oracle and product, and
the mixing script end to end."""
import os

import pytest
import torch

from controllora_amd import kernels as K
from tests import full_cases as F
from tests import lora_fold_cases as L

pytestmark = pytest.mark.gpu
f16 = torch.float16
REAL = dict(B=2, side=16, C=320, heads=8, ctx=768, ctrl_c=256)       # as test_pre_post_lora_chain_on_gpu's real-width run


@pytest.mark.parametrize("rank", [4, 8, 256])
def test_fold_kernel_all_sd15_sites_in_one_launch(rank):
    dev = "cuda"
    segs = L.sd15_site_segments()
    assert len(segs) == 32 * 4
    Ws, mems, outs, jobs = [], [], [], []
    for i, (rows, Kd) in enumerate(segs):
        W, mem = L.fold_inputs(rows, Kd, [(rank, 0.7)], seed=100 + i, dev=dev)
        out, out_t = torch.full_like(W, float("nan")), torch.full((Kd, rows), float("nan"), dtype=f16, device=dev)
        Ws.append(W); mems.append(mem); outs.append((out, out_t))
        jobs.append(K.lora_fold_job(W, out, out_t, mem))
    K.lora_fold_multi(jobs)
    torch.cuda.synchronize()
    first = [(o.clone(), t.clone()) for o, t in outs]
    K.lora_fold_multi(jobs)                                  # a repeat launch is bit-identical
    torch.cuda.synchronize()
    differ, elems, worst_share = 0, 0, 0.0
    for W, mem, (out, out_t), (o1, t1) in zip(Ws, mems, outs, first):
        assert torch.equal(out, o1) and torch.equal(out_t, t1)
        assert torch.equal(out_t, out.t()), "transposed operand is not the forward operand's transpose"
        d = L.ulp_distance(out, L.fold_reference(W, mem))
        assert int(d.max()) <= 1, (tuple(W.shape), int(d.max()))
        share = float((d > 0).float().mean())
        assert share <= L.MAX_DIFFER, (tuple(W.shape), share)
        worst_share = max(worst_share, share)
        differ += int((d > 0).sum()); elems += d.numel()
    print(f"FOLD_KERNEL_SD15 rank {rank}: {len(jobs)} jobs, {elems} elements, {differ} differ from the fp64 fold by one ulp "
          f"(share {differ / elems:.2e}, worst job {worst_share:.2e}, cap {L.MAX_DIFFER})")
    for i in (0, 5, 63, 127):                                # the same jobs launched one by one
        a, a_t = L.run_fold(Ws[i], mems[i])
        assert torch.equal(a, outs[i][0]) and torch.equal(a_t, outs[i][1])


def test_fold_kernel_copy_zero_members_and_stacked_members():
    dev = "cuda"
    W, mem = L.fold_inputs(1280, 768, [(4, 0.7), (16, 1.0), (8, 0.5)], seed=7, dev=dev)
    cp, cp_t = L.run_fold(W, [])
    assert torch.equal(cp, W) and torch.equal(cp_t, W.t())
    z, z_t = L.run_fold(W, [(torch.zeros_like(u), d, s) for u, d, s in mem])
    assert torch.equal(z, W) and torch.equal(z_t, W.t())
    L.check_fold_against_fp64(1280, 768, [(4, 0.7), (16, 1.0), (8, 0.5)], seed=7, dev=dev)
    L.check_fold_against_fp64(1280, 1280, [(16, 1.0)], up_std=0.2, dev=dev)
    L.check_fold_against_fp64(48, 32, [(4, 0.7)], up_std=0.05, dev=dev)


@pytest.mark.parametrize("arrangement", L.ARRANGEMENTS)
@pytest.mark.parametrize("kind", L.KINDS)
def test_folded_site_matches_oracle_chain_at_a_real_width(kind, arrangement):
    L.check_fold_site(kind, arrangement, "cuda", **REAL)


@pytest.mark.parametrize("kind", ["v1", "v2"])
def test_training_a_control_lora_on_a_folded_base_at_a_real_width(kind):
    L.check_fold_training(kind, "cuda", **REAL)


def _assert_all_folded(p_clora, members):
    rep = p_clora.fold_report()
    assert rep and all(r["folded"] and r["members"] == members for r in rep.values()), rep


def test_mixed_folded_ddim_small_50_steps():
    """test_ddim_denoised_latents_small_50_steps with every site mixed (pre) and folded, held to that test's limits"""
    o_unet, o_clora, p_unet, p_clora, _ = L.mixed_small_pair("cuda", "v1", pre=True, post=False)
    _assert_all_folded(p_clora, 1)
    r = F.ddim_parity(o_unet, o_clora, p_unet, p_clora, "cuda", res=128, steps=50, guidance_scale=9.0, nb=2, ctx_dim=64, ctx_len=7,
                      fp16_floor=True)
    print("MIXED_FOLDED DDIM_LATENT_PARITY small 50 steps", r)
    assert r["latents"] < 5.5e-3 and r["latents"] < r["fp16_oracle_vs_fp32_oracle"] * 1.1, r


@pytest.mark.parametrize("graph", [False, True])
def test_mixed_folded_dpm_solver_30_steps(graph):
    """test_validation_sampling_loop_dpm_solver_30_steps with every site mixed (pre and post) and folded, same limits"""
    o_unet, o_clora, p_unet, p_clora, _ = L.mixed_small_pair("cuda", "v1", pre=True, post=True)
    _assert_all_folded(p_clora, 2)
    r = F.ddim_parity(o_unet, o_clora, p_unet, p_clora, "cuda", res=128, steps=30, guidance_scale=7.5, nb=1, ctx_dim=64, ctx_len=7,
                      fp16_floor=True, sampler="dpm", graph=graph)
    print("MIXED_FOLDED VALIDATION_DPM30_LATENT_PARITY small", "graph" if graph else "eager", r)
    assert r["latents"] < 5.5e-3 and r["latents"] < r["fp16_oracle_vs_fp32_oracle"] * 1.1, r


def test_mixed_folded_ddim_full_topology():
    """test_ddim_denoised_latents_full_topology with every one of the 32 sites mixed (pre) and folded, same limit"""
    from controllora_amd import loading, models as M
    o_unet, o_clora, p_unet, p_clora = F.build_pair("fill50k.json", "cuda")
    sd, o_members = L.lora_state_dict(o_unet, None, rank=4, seed=31, up_std=0.02)
    L.mix_oracle(o_unet, o_clora, o_members, pre=True, post=False)
    M.mix_lora_into_control_lora(p_unet, p_clora, loading.load_lora_attn_procs(p_unet, sd), pre=True, post=False, fold=True)
    _assert_all_folded(p_clora, 1)
    assert len(p_clora.fold_report()) == 32
    with L.count_library_calls() as names:
        assert p_clora.fold_now(p_unet, scale=1.0) == 32
    assert names == ["clora_lora_fold_f16"], names
    r = F.ddim_parity(o_unet, o_clora, p_unet, p_clora, "cuda", res=256, steps=6, guidance_scale=9.0, nb=1)
    print("MIXED_FOLDED DDIM_LATENT_PARITY sd15 6 steps", r)
    assert r["latents"] < 7.5e-3, r


def test_mixing_script_writes_guide_image_strips(tmp_path, monkeypatch):
    import numpy as np
    from PIL import Image
    from controllora_amd import models as M
    from oracle import cases
    import mix_lora_and_control_lora as script
    torch.manual_seed(3)
    clora = M.ControlLoRA(**cases.CASES["v1"])
    with torch.no_grad():
        for n, q in clora.named_parameters():
            if ".up.weight" in n:
                q.normal_(0.0, 0.05)
    clora.save_pretrained(str(tmp_path / "clora"))
    monkeypatch.chdir(tmp_path)
    common = ["--pretrained_model_name_or_path", "random:small", "--control_lora", str(tmp_path / "clora"), "--lora", "random:3",
              "--dataset_name", "synthetic:fill50k", "--resolution", "64", "--validation_prompt", "red circle with blue background",
              "--num_validation_images", "2", "--inject_post_lora", "--lora_std", "0.2"]
    script.main(common + ["--output_dir", "mixed"])
    script.main(common[:-1] + ["0.0", "--output_dir", "zeroed"])
    for i in range(2):
        a = np.asarray(Image.open(tmp_path / "samples" / "mixed" / f"{i}.png"))
        b = np.asarray(Image.open(tmp_path / "samples" / "zeroed" / f"{i}.png"))
        assert a.shape == b.shape == (64, 128, 3), a.shape               # [guide | image]
        assert np.array_equal(a[:, :64], b[:, :64]) and a[:, :64].max() == 255, "the left half is the guide"
        assert not np.array_equal(a[:, 64:], b[:, 64:]), "the LoRA must change the image"
    assert sorted(os.listdir(tmp_path / "samples" / "mixed")) == ["0.png", "1.png"]
