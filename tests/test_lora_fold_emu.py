"""CPU tests of folding frozen chained LoRAs into the frozen attention weights, on the emulated kernels: the fold kernel
(clora_lora_fold_f16) against an fp64 fold, the folded site against the oracle's chain, training on a folded base, fallbacks and
stale-cache behaviour, launch counts of a whole mixed UNet, and the loader of diffusers-format LoRA files."""
import copy
import os

import pytest
import torch

from controllora_amd import kernels as K, loading, models as M
from tests import lora_fold_cases as L
from tests.emu_fixture import use_emulator

f16 = torch.float16


@pytest.fixture(autouse=True)
def _emu():
    with use_emulator():
        yield


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("rows,Kd,members,up_std", [
    (320, 320, [(4, 0.7)], 0.02),
    (640, 768, [(4, 0.7), (8, 1.0)], 0.02),                  # a k / v segment of a cross-attention site, two stacked members
    (320, 320, [(256, 0.7)], 0.02),                          # rank 256
    (1280, 1280, [(16, 1.0)], 0.2),                          # a large delta
    (48, 32, [(4, 0.7), (1, 1.0), (8, 0.5), (4, 1.0)], 0.05),    # the small test topology's sizes: not multiples of the tile
    (72, 64, [(4, 0.7)], 0.05),
])
def test_fold_kernel_matches_fp64_fold(rows, Kd, members, up_std):
    L.check_fold_against_fp64(rows, Kd, members, up_std=up_std)


def test_fold_kernel_invariants():
    W, mem = L.fold_inputs(136, 200, [(4, 0.7), (8, 1.0)], seed=3)
    out, out_t = L.run_fold(W, mem)
    out2, out_t2 = L.run_fold(W, mem)
    assert torch.equal(out, out2) and torch.equal(out_t, out_t2), "a repeat launch is not bit-identical"
    assert torch.equal(out_t, out.t()) and not torch.equal(out, W)
    cp, cp_t = L.run_fold(W, [])
    assert torch.equal(cp, W) and torch.equal(cp_t, W.t()), "a member-less job is a copy"
    zero = [(torch.zeros_like(u), d, s) for u, d, s in mem]
    z, z_t = L.run_fold(W, zero)
    assert torch.equal(z, W) and torch.equal(z_t, W.t()), "zero up matrices give back W"
    fwd_only, none_t = L.run_fold(W, mem, transposed=False)
    assert none_t is None and torch.equal(fwd_only, out)


def test_fold_kernel_several_jobs_in_one_launch_equal_single_launches():
    shapes = [(64, 32, [(4, 0.7)]), (32, 48, []), (128, 64, [(8, 1.0), (4, 0.3)]), (40, 136, [(16, 0.7)]), (96, 96, [(4, 1.0)] * 8)]
    singles, jobs, outs = [], [], []
    for i, (rows, Kd, members) in enumerate(shapes):
        W, mem = L.fold_inputs(rows, Kd, members, seed=10 + i)
        singles.append(L.run_fold(W, mem))
        out, out_t = torch.zeros_like(W), torch.zeros((Kd, rows), dtype=f16)
        jobs.append(K.lora_fold_job(W, out, out_t, mem))
        outs.append((out, out_t))
    K.lora_fold_multi(jobs)
    for (a, a_t), (b, b_t) in zip(singles, outs):
        assert torch.equal(a, b) and torch.equal(a_t, b_t)


def test_fold_job_writes_row_segments_of_a_packed_operand():
    """the way the host stack uses it: q | k | v segments of one [3C, C] pack and column slices of its [C, 3C] dgrad operand"""
    C = 40
    W, _ = L.fold_inputs(3 * C, C, [], seed=1)
    out, out_t = torch.zeros_like(W), torch.zeros((C, 3 * C), dtype=f16)
    mems = [L.fold_inputs(C, C, m, seed=2 + i)[1] for i, m in enumerate(([(4, 0.7)], [], [(8, 1.0), (4, 0.7)]))]
    K.lora_fold_multi([K.lora_fold_job(W[i * C:(i + 1) * C], out[i * C:(i + 1) * C], out_t[:, i * C:(i + 1) * C], mems[i]) for i in range(3)])
    ref = torch.cat([L.fold_reference(W[i * C:(i + 1) * C], mems[i]) for i in range(3)], 0)
    assert int(L.ulp_distance(out, ref).max()) <= 1 and torch.equal(out[C:2 * C], W[C:2 * C]) and torch.equal(out_t, out.t())
    with pytest.raises(Exception):
        K.lora_fold_job(W, out, out_t, [(torch.zeros(3 * C, 4), torch.zeros(4, C), 1.0)] * 9)     # more members than a job holds


# ------------------------------------------------------------------------------------------------ site
@pytest.mark.parametrize("arrangement", L.ARRANGEMENTS)
@pytest.mark.parametrize("kind", L.KINDS)
def test_folded_site_matches_oracle_chain(kind, arrangement):
    L.check_fold_site(kind, arrangement, "cpu")


@pytest.mark.parametrize("kind", ["v1", "v2"])
def test_training_a_control_lora_on_a_folded_base(kind):
    L.check_fold_training(kind, "cpu")


# ------------------------------------------------------------------------------------------------ fallbacks and staleness
def _fold_out(s, p_main=None, **kw):
    with torch.no_grad():
        return L.product_site(s, p_main, **kw)[0]


def _fresh(s, p_main=None):
    """the same site folded from scratch: a deep copy of the processors without any cached fold"""
    p = copy.deepcopy(s["p_main"] if p_main is None else p_main)
    p.__dict__.pop("_fold", None)
    return p


@pytest.mark.parametrize("self_attn", [True, False])
def test_ineligible_chains_and_empty_chains_are_untouched_by_the_switch(self_attn):
    for what in ("post_add member", "control member", "trainable member under autograd", "empty chain"):
        s = L.build_site("v1", self_attn, "both", "cpu")
        p = s["p_main"]
        cad = p.cross_attention_dim
        grad = False
        if what == "post_add member":
            extra = M.LoRACrossAttnProcessor(64, cad, rank=4, post_add=True)
            torch.nn.init.normal_(extra.to_q_lora.up.weight, std=0.05)
            p.inject_post_lora(extra)
        elif what == "control member":
            p.post_loras[0] = copy.deepcopy(p)
            p.post_loras[0].pre_loras, p.post_loras[0].post_loras = [], []
            p.post_loras[0].inject_control_states(s["ctrl"].permute(0, 2, 3, 1).reshape(s["B"], s["N"], -1).contiguous())
        elif what == "trainable member under autograd":
            grad = True
        else:
            p.pre_loras, p.post_loras = [], []
        p.fold_chain = False
        off = L.product_site(s, grad=grad)[0].detach()
        p.fold_chain = True
        with torch.set_grad_enabled(grad):
            assert p._fold_blocker() is not None and (what == "empty chain" or p._needs_generic_path()), what
        on = L.product_site(s, grad=grad)[0].detach()
        assert torch.equal(on, off), what
        assert "_fold" not in p.__dict__, what


@pytest.mark.parametrize("self_attn", [True, False])
def test_a_stale_fold_is_never_served(self_attn):
    s = L.build_site("v1", self_attn, "two_post", "cpu")
    p = s["p_main"]
    p.fold_chain = True
    y0 = _fold_out(s)
    assert torch.equal(y0, _fold_out(s)) and torch.equal(y0, _fold_out(s, _fresh(s)))
    gen0 = p.__dict__["_fold"]["gen"]
    _fold_out(s)
    assert p.__dict__["_fold"]["gen"] == gen0, "an unchanged site must not refold"
    member = p.post_loras[0]
    with torch.no_grad():                                   # in-place update of a member
        member.to_q_lora.up.weight.mul_(-1.5)
    y1 = _fold_out(s)
    assert not torch.equal(y1, y0) and torch.equal(y1, _fold_out(s, _fresh(s)))
    other = M.LoRACrossAttnProcessor(64, p.cross_attention_dim, rank=8)       # load_state_dict into a member
    from oracle import cases
    cases.seeded_weights_(other, seed=77)
    member.load_state_dict(other.state_dict())
    y2 = _fold_out(s)
    assert not torch.equal(y2, y1) and torch.equal(y2, _fold_out(s, _fresh(s)))
    y3 = _fold_out(s, scale=0.3)                            # another scale
    assert not torch.equal(y3, y2) and torch.equal(y3, _fold_out(s, _fresh(s), scale=0.3))
    assert torch.equal(_fold_out(s), y2)
    p.post_loras.reverse()                                  # the chain reordered
    assert torch.equal(_fold_out(s), _fold_out(s, _fresh(s)))
    p.post_loras.clear()                                    # the chain cleared: the unfolded site, bit for bit
    bare = _fresh(s)
    bare.fold_chain = False
    y5 = _fold_out(s)
    assert torch.equal(y5, _fold_out(s, bare)) and not torch.equal(y5, y2)


def test_the_text_kv_cache_never_serves_another_folds_projections():
    s = L.build_site("v1", False, "two_post", "cpu")
    p = s["p_main"]
    p.fold_chain = True
    e = s["e"].clone()                                      # one embedding tensor for every call: the cache key's storage / version
    with M.text_kv_cache():
        y0 = _fold_out(s, e=e)
        assert torch.equal(y0, _fold_out(s, e=e))
        assert len(M._TEXT_KV) == 1
        p.post_loras.reverse()
        y1 = _fold_out(s, e=e)
        with M.text_kv_cache():                             # (an empty cache of its own for the reference value)
            assert torch.equal(y1, _fold_out(s, _fresh(s), e=e))
        members = list(p.post_loras)
        p.post_loras.clear()
        y2 = _fold_out(s, e=e)
        bare = _fresh(s)
        bare.fold_chain = False
        with M.text_kv_cache():
            assert torch.equal(y2, _fold_out(s, bare, e=e))
        assert not torch.equal(y2, y0)
        p.post_loras.extend(members)                        # and back: the cached projections of that fold are valid again
        assert torch.equal(_fold_out(s, e=e), y1)


# ------------------------------------------------------------------------------------------------ whole UNet: launches, loader
def _unet_forward(unet, clora, inp):
    with torch.no_grad():
        clora(inp["guide"][:1].half())
        return unet(inp["latents"].half(), 501, inp["ehs"].half()).sample


def test_folded_mixed_unet_issues_the_plain_unets_launches(tmp_path):
    from oracle import cases
    from tests.e2e_cases import build_product_case
    inp = cases.seeded_inputs()
    plain_unet, _, plain_clora = build_product_case("v1", "cpu")
    _, _, unet, clora, sd = L.mixed_small_pair("cpu", "v1", pre=True, post=False, fold=True)
    rep = clora.fold_report()
    assert len(rep) == len(unet.attn_processors) and all(r["folded"] and r["members"] == 1 for r in rep.values()), rep
    counts, outs = {}, {}
    for tag, (u, c) in (("plain", (plain_unet, plain_clora)), ("folded", (unet, clora))):
        _unet_forward(u, c, inp)                                       # warm: lazy packs, the fold itself
        with L.count_library_calls() as names:
            outs[tag] = _unet_forward(u, c, inp)
        counts[tag] = len(names)
        assert "clora_lora_fold_f16" not in names
    clora.fold_chains(False)
    assert not any(r["folded"] for r in clora.fold_report().values())
    _unet_forward(unet, clora, inp)
    with L.count_library_calls() as names:
        outs["generic"] = _unet_forward(unet, clora, inp)
    counts["generic"] = len(names)
    print("LAUNCHES small topology, one UNet forward + hint encoder:", counts)
    assert counts["folded"] == counts["plain"] < counts["generic"], counts
    assert not torch.equal(outs["folded"], outs["plain"])
    e = L.rel(outs["folded"], outs["generic"])
    print("folded vs generic mixed forward rel-L2", e, " mixed vs plain", L.rel(outs["folded"], outs["plain"]))
    assert 4 * e < L.rel(outs["folded"], outs["plain"])         # the two mixed paths agree far better than mixing moves the output
    # one launch folds every site of the model
    clora.fold_chains(True)
    with L.count_library_calls() as names:
        n = clora.fold_now(unet, scale=0.5)
    assert n == len(rep) and names == ["clora_lora_fold_f16"], (n, names)


def test_loader_reads_diffusers_format_lora_files(tmp_path):
    from oracle import cases
    from tests.e2e_cases import build_product_case
    o_unet, _, _ = cases.build_oracle_case("v1")
    unet, _, clora = build_product_case("v1", "cpu")
    sd, o_members = L.lora_state_dict(o_unet, None, rank=6)
    torch.save(sd, tmp_path / "pytorch_lora_weights.bin")
    os.makedirs(tmp_path / "st")
    from safetensors.torch import save_file
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "st" / "diffusion_pytorch_model.safetensors"))
    torch.save(sd, tmp_path / "st" / "other_name.bin")
    loaded = [loading.load_lora_attn_procs(unet, src) for src in
              (sd, str(tmp_path / "pytorch_lora_weights.bin"), str(tmp_path), str(tmp_path / "st"), str(tmp_path / "st" / "other_name.bin"))]
    names = list(unet.attn_processors.keys())
    for procs in loaded:
        assert list(procs) == names
        for n in names:
            p, o = procs[n], o_members[n]
            assert type(p) is M.LoRACrossAttnProcessor and p.rank == 6 and p.hidden_size == o.hidden_size
            assert p.cross_attention_dim == o.cross_attention_dim and not p.post_add
            for k, v in o.state_dict().items():
                assert torch.equal(p.state_dict()[k], v), (n, k)
    short = dict(sd)
    gone = sorted(short)[3]
    del short[gone]
    with pytest.raises(ValueError, match="missing.*" + gone.replace(".", r"\.")):
        loading.load_lora_attn_procs(unet, short)
    with pytest.raises(ValueError, match="unexpected.*not_a_site"):
        loading.load_lora_attn_procs(unet, dict(sd, **{"not_a_site.processor.to_q_lora.up.weight": torch.zeros(1)}))
    with pytest.raises(FileNotFoundError):
        loading.load_lora_attn_procs(unet, str(tmp_path / "st" / "nothing_here"))
    # injected through the loader == injected by hand
    inp = cases.seeded_inputs()
    M.mix_lora_into_control_lora(unet, clora, loaded[1], pre=True, post=True, fold=True)
    unet2, _, clora2 = build_product_case("v1", "cpu")
    for n, proc in M.map_processors_to_unet(unet2, clora2).items():
        hand = M.LoRACrossAttnProcessor(o_members[n].hidden_size, o_members[n].cross_attention_dim, rank=6)
        hand.load_state_dict(o_members[n].state_dict())
        hand.requires_grad_(False)
        proc.inject_pre_lora(hand)
        proc.inject_post_lora(hand)
    clora2.fold_chains(True)
    assert all(r["folded"] and r["members"] == 2 for r in clora.fold_report().values())
    assert torch.equal(_unet_forward(unet, clora, inp), _unet_forward(unet2, clora2, inp))
    with pytest.raises(ValueError, match="no LoRA processor"):
        M.mix_lora_into_control_lora(unet2, clora2, {})
