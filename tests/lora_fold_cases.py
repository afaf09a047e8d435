"""Shared cases of the LoRA-fold tests (CPU on the emulated kernels, GPU on the real library): the fold kernel against an fp64
fold, one attention site with frozen plain LoRAs chained on against the oracle's chain (oracle/controllora_ref.py), training a
ControlLoRA on a folded base, and whole UNets with every site mixed identically in oracle and product."""
import contextlib
import copy

import torch

from controllora_amd import capi, kernels as K, loading, models as M, unet as U
from oracle import cases, controllora_ref as cr, unet_ref
from tests.e2e_cases import rel

f16, f32 = torch.float16, torch.float32
SCALE = 0.7
# tests/e2e_cases.check_pre_post_chain's limits: what the generic path of the same chains is held to
TOL_Y, TOL_DH, TOL_DC, TOL_W = 4e-3, 1e-2, 2e-2, 3e-2
# share of elements that may differ at all from the fp64 fold rounded to fp16 (and then by one ulp): a cap, not a tolerance --
# torch's own fp32 fold differs in at most 2.6e-4 of the elements on these shapes
MAX_DIFFER = 1e-3


# ------------------------------------------------------------------------------------------------ kernel
def fold_inputs(rows, Kd, members, seed=0, up_std=0.02, w_std=0.05, dev="cpu"):
    """members: [(rank, scale)] -> W fp16 [rows, K], [(up fp32, down fp32, scale)]"""
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(rows, Kd, generator=g) * w_std).half().to(dev)
    mem = [((torch.randn(rows, r, generator=g) * up_std).to(dev), (torch.randn(r, Kd, generator=g) / r).to(dev), s) for r, s in members]
    return W, mem


def fold_reference(W, mem):
    """the fold in fp64 (the scale as the fp32 value the kernel is handed), rounded to fp16 once"""
    ref = W.double()
    for up, down, s in mem:
        ref = ref + float(torch.tensor(s, dtype=f32)) * (up.double() @ down.double())
    return ref.half().cpu()


def ulp_distance(a, b):
    """distance in fp16 steps between two fp16 tensors (sign-magnitude -> a monotonic integer line)"""
    def line(t):
        i = t.cpu().contiguous().view(torch.int16).int()
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (line(a) - line(b)).abs()


def run_fold(W, mem, transposed=True):
    out = torch.full_like(W, float("nan"))
    out_t = torch.full((W.shape[1], W.shape[0]), float("nan"), dtype=f16, device=W.device) if transposed else None
    K.lora_fold_multi([K.lora_fold_job(W, out, out_t, mem)])
    return out, out_t


def check_fold_against_fp64(rows, Kd, members, seed=0, up_std=0.02, dev="cpu"):
    W, mem = fold_inputs(rows, Kd, members, seed, up_std, dev=dev)
    out, out_t = run_fold(W, mem)
    ref = fold_reference(W, mem)
    d = ulp_distance(out, ref)
    stats = dict(shape=(rows, Kd), members=members, differ=float((d > 0).float().mean()), max_ulp=int(d.max()),
                 moved=float((ref != W.cpu()).float().mean()))
    print("FOLD_VS_FP64", stats)
    assert stats["differ"] <= MAX_DIFFER, stats
    assert stats["max_ulp"] <= 1, stats
    assert stats["moved"] > 0.5, ("the case must move the weights", stats)
    assert torch.equal(out_t, out.t()), "transposed operand is not the forward operand's transpose"
    return stats


def sd15_site_segments():
    """(rows, K) of every fold segment of SD-1.5's 32 attention sites: q, k, v, out of the 16 self- and 16 cross-attention sites"""
    widths = [320] * 2 + [640] * 2 + [1280] * 2 + [1280] + [1280] * 3 + [640] * 3 + [320] * 3
    segs = []
    for C in widths:
        segs += [(C, C)] * 4                              # attn1: q, k, v, out
        segs += [(C, C), (C, 768), (C, 768), (C, C)]      # attn2: q, k (text), v (text), out
    return segs


# ------------------------------------------------------------------------------------------------ one site
KINDS = ("v1", "v1_concat", "v2")
ARRANGEMENTS = ("pre", "post", "both", "two_post")


def _mains(kind, C, cad, ctrl_c):
    if kind == "v1":
        return cr.ControlLoRAProcRef(C, cad, rank=4), M.ControlLoRACrossAttnProcessor(C, cad, rank=4), C
    if kind == "v1_concat":
        kw = dict(rank=4, concat_hidden=True, control_channels=ctrl_c)
        return cr.ControlLoRAProcRef(C, cad, **kw), M.ControlLoRACrossAttnProcessor(C, cad, **kw), ctrl_c
    return (cr.ControlLoRAProcV2Ref(C, cad, rank=4, control_channels=ctrl_c),
            M.ControlLoRACrossAttnProcessorV2(C, cad, rank=4, control_channels=ctrl_c), ctrl_c)


def _member_pair(C, cad, rank, seed, dev, skip=None):
    """a plain LoRA in oracle and product form with the same seeded weights; skip: 'value' / 'output' sets that member's own flag
    (the adapter exists and is non-zero: leaving it out is what the flag must do)"""
    o, p = cr.LoRAProcRef(C, cad, rank=rank), M.LoRACrossAttnProcessor(C, cad, rank=rank)
    cases.seeded_weights_(o, seed=seed)
    p.load_state_dict(o.state_dict())
    p.to(dev)
    for m in (o, p):
        if skip == "value":
            m.skip_value_states(True)
        elif skip == "output":
            m.skip_output_states(True)
    return o, p


def build_site(kind, self_attn, arrangement, dev, C=64, heads=4, ctx=48, ctrl_c=32, B=2, side=4, seed=0):
    torch.manual_seed(seed)
    N = side * side
    cad = None if self_attn else ctx
    o_attn = unet_ref.CrossAttention(C, cad, heads=heads, dim_head=C // heads)
    cases.seeded_weights_(o_attn, seed=5)
    p_attn = U.CrossAttention(C, cad, heads=heads, dim_head=C // heads)
    with torch.no_grad():
        for k, v in p_attn.state_dict().items():
            v.copy_(o_attn.state_dict()[k].to(v.dtype))
        for q in o_attn.parameters():                      # oracle: fp32 math on fp16-rounded frozen weights
            q.data = q.data.half().float()
    p_attn.to(dev)
    o_main, p_main, cc = _mains(kind, C, cad, ctrl_c)
    cases.seeded_weights_(o_main, seed=1)
    p_main.load_state_dict(o_main.state_dict())
    p_main.to(dev)
    A = _member_pair(C, cad, 4, 2, dev)
    Bv = _member_pair(C, cad, 8, 3, dev, skip="value")
    Co = _member_pair(C, cad, 4, 4, dev, skip="output")
    pre, post = {"pre": ([Bv], []), "post": ([], [Co]), "both": ([A], [Bv]), "two_post": ([], [Bv, Co])}[arrangement]
    for o, p in pre:
        o_main.inject_pre_lora(o); p_main.inject_pre_lora(p)
    for o, p in post:
        o_main.inject_post_lora(o); p_main.inject_post_lora(p)
    h = torch.randn(B, N, C).half()
    e = None if self_attn else torch.randn(B, 5, ctx).half()
    ctrl = torch.randn(B, cc, side, side).half()
    go = torch.randn(B, N, C).half()
    return dict(o_attn=o_attn, p_attn=p_attn, o_main=o_main, p_main=p_main, h=h, e=e, ctrl=ctrl, go=go, B=B, N=N, dev=dev,
                p_members=[p for _, p in pre + post], o_members=[o for o, _ in pre + post])


def oracle_site(s, o_main=None, grad=False):
    o_main = s["o_main"] if o_main is None else o_main
    ho = s["h"].float().requires_grad_(grad)
    co = s["ctrl"].float().requires_grad_(grad)
    o_main.inject_control_states(co)
    with torch.set_grad_enabled(grad):
        yo = o_main(s["o_attn"], ho, None if s["e"] is None else s["e"].float(), None, SCALE)
    return yo, ho, co


def product_site(s, p_main=None, scale=SCALE, grad=False, e=None):
    p_main = s["p_main"] if p_main is None else p_main
    dev = s["dev"]
    hp = s["h"].clone().to(dev).requires_grad_(grad)
    cp = s["ctrl"].permute(0, 2, 3, 1).reshape(s["B"], s["N"], -1).contiguous().to(dev).requires_grad_(grad)
    p_main.inject_control_states(cp)
    if e is None and s["e"] is not None:
        e = s["e"].to(dev)
    with torch.set_grad_enabled(grad):
        yp = p_main(s["p_attn"], hp, e, None, scale)
    return yp, hp, cp


def wrong_quirk_oracles(s):
    """the oracle chain evaluated with each scaling quirk broken, as deep copies of the oracle processors:
    'value_scale': every member's value adapter scaled by `scale` instead of 1.0 (its up matrix pre-multiplied);
    'skip': every member's skip flag cleared, so a segment that member leaves out is applied"""
    out = {}
    o = copy.deepcopy(s["o_main"])
    members = o.pre_loras + o.post_loras
    live_v = [m for m in members if not m.value_states_skipped]
    if live_v:
        with torch.no_grad():
            for m in live_v:
                m.to_v_lora.up.weight.mul_(SCALE)
        out["value_scale"] = o
    o = copy.deepcopy(s["o_main"])
    members = o.pre_loras + o.post_loras
    if any(m.value_states_skipped or m.output_states_skipped for m in members):
        for m in members:
            m.value_states_skipped = m.output_states_skipped = False
        out["skip"] = o
    return out


def check_fold_site(kind, arrangement, dev, **shape):
    """folded site vs the oracle chain, no autograd; the generic path's error beside it; the case tells the quirks apart"""
    worst = {}
    for self_attn in (True, False):
        s = build_site(kind, self_attn, arrangement, dev, **shape)
        yo, _, _ = oracle_site(s)
        s["p_main"].fold_chain = True
        assert s["p_main"]._fold_blocker() is None or torch.is_grad_enabled()
        with torch.no_grad():
            y_fold, _, _ = product_site(s)
            assert not s["p_main"]._needs_generic_path(), s["p_main"]._fold_blocker()
            s["p_main"].fold_chain = False
            y_gen, _, _ = product_site(s)
        e_fold, e_gen = rel(y_fold, yo), rel(y_gen, yo)
        tag = f"{kind}/{arrangement}/{'self' if self_attn else 'cross'}"
        print(f"FOLD_SITE {tag}: folded {e_fold:.3e}  generic {e_gen:.3e}  (limit {TOL_Y})")
        wrong = {k: rel(oracle_site(s, o)[0], yo) for k, o in wrong_quirk_oracles(s).items()}
        print(f"FOLD_SITE {tag}: oracle with a quirk broken sits", {k: f"{v:.3e}" for k, v in wrong.items()}, "away")
        assert wrong, "every arrangement carries a member the quirks act on"
        for k, v in wrong.items():
            assert v > 2 * TOL_Y, (tag, k, v, "the case cannot tell this quirk apart")
        assert e_fold < TOL_Y, (tag, e_fold)
        worst[tag] = (e_fold, e_gen)
    return worst


def check_fold_training(kind, dev, **shape):
    """a trainable main processor on frozen, folded members under autograd: output, d(hidden), d(control) and the main
    processor's weight gradients vs the oracle chain; members get no gradient"""
    worst = {}
    for self_attn in (True, False):
        s = build_site(kind, self_attn, "both", dev, **shape)
        yo, ho, co = oracle_site(s, grad=True)
        yo.backward(s["go"].float())
        for m in s["p_members"]:
            m.requires_grad_(False)
        s["p_main"].fold_chain = True
        assert s["p_main"]._fold_blocker() is None and not s["p_main"]._needs_generic_path()
        yp, hp, cp = product_site(s, grad=True)
        yp.backward(s["go"].to(dev))
        errs = {"y": rel(yp, yo.detach()), "dh": rel(hp.grad, ho.grad),
                "dctrl": rel(cp.grad, co.grad.permute(0, 2, 3, 1).reshape(s["B"], s["N"], -1)), "dw": 0.0}
        for (n, a), (_, b_) in zip(s["p_main"].named_parameters(), s["o_main"].named_parameters()):
            if b_.grad is not None and float(b_.grad.norm()) > 0:
                assert a.grad is not None, n
                errs["dw"] = max(errs["dw"], rel(a.grad, b_.grad))
        print(f"FOLD_TRAIN {kind}/{'self' if self_attn else 'cross'}:", {k: f"{v:.3e}" for k, v in errs.items()})
        assert errs["y"] < TOL_Y and errs["dh"] < TOL_DH and errs["dctrl"] < TOL_DC and 0 < errs["dw"] < TOL_W, errs
        assert all(q.grad is None for m in s["p_members"] for q in m.parameters())
        for k, v in errs.items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


# ------------------------------------------------------------------------------------------------ whole UNets
@contextlib.contextmanager
def count_library_calls():
    """counts the calls into the loaded kernel library (every call is one launch group of the C ABI)"""
    lib = capi.lib()
    names = []
    orig = lib.call

    def call(name, *args):
        names.append(name)
        return orig(name, *args)

    lib.call = call
    try:
        yield names
    finally:
        del lib.call


def lora_state_dict(o_unet, hidden_of, rank=4, seed=21, up_std=0.05):
    """a diffusers-format LoRA state dict (`<site>.processor.to_*_lora.{down,up}.weight`) with seeded non-zero weights for every
    attention site of the oracle UNet, plus the oracle processors that carry the same weights -> (state dict, {name: LoRAProcRef})"""
    sd, procs = {}, {}
    for i, name in enumerate(o_unet.attn_processors.keys()):
        site = o_unet.get_submodule(name[:-len(".processor")])
        hidden = site.to_q.weight.shape[0]
        cad = None if name.endswith("attn1.processor") else site.to_k.weight.shape[1]
        o = cr.LoRAProcRef(hidden, cad, rank=rank)
        cases.seeded_weights_(o, seed=seed + i, up_std=up_std)
        procs[name] = o
        for k, v in o.state_dict().items():
            sd[f"{name}.{k}"] = v.clone()
    return sd, procs


def mix_oracle(o_unet, o_clora, o_members, pre=True, post=False):
    """the reference's injection (mix_lora_and_control_lora.py:111-121) on the oracle processors.  The members are also registered
    as submodules of their site's processor so that module-wide casts / moves / copies of the oracle reach them."""
    for name, proc in cr.map_processors_to_unet(o_unet, o_clora).items():
        m = o_members[name]
        if pre:
            proc.inject_pre_lora(m)
        if post:
            proc.inject_post_lora(m)
        proc.add_module("mixed_member", m)
    o_unet.set_attn_processor(cr.map_processors_to_unet(o_unet, o_clora))


def mixed_small_pair(dev, case="v1", pre=True, post=False, fold=True):
    """small topology, every site mixed identically in oracle and product (the product through the loader and
    models.mix_lora_into_control_lora) -> (o_unet, o_clora, p_unet, p_clora, lora state dict)"""
    from tests.e2e_cases import build_product_case
    o_unet, _, o_clora = cases.build_oracle_case(case)
    p_unet, _, p_clora = build_product_case(case, dev)
    with torch.no_grad():
        for p in o_unet.parameters():                      # frozen weights: fp16 values on both sides
            p.copy_(p.half().float())
    sd, o_members = lora_state_dict(o_unet, None)
    mix_oracle(o_unet, o_clora, o_members, pre, post)
    M.mix_lora_into_control_lora(p_unet, p_clora, loading.load_lora_attn_procs(p_unet, sd), pre=pre, post=post, fold=fold)
    return o_unet, o_clora, p_unet, p_clora, sd
