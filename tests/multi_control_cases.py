"""Shared cases of the multi-ControlLoRA tests (CPU on the emulated kernels, GPU on the real library): the control-mix kernel
(clora_control_mix_q_f16) against an fp64 evaluation, one v1 attention site with frozen control members chained on against the
oracle's chain (oracle/controllora_ref.py), the recorded reference outputs (tests/golden/multi_control_records.safetensors), and
whole small UNets steered by two control models."""
import copy
import ctypes
import os

import torch

from controllora_amd import capi, kernels as K, models as M, unet as U
from oracle import cases, controllora_ref as cr, unet_ref
from tests.e2e_cases import rel
from tests.lora_fold_cases import SCALE, TOL_Y, count_library_calls, ulp_distance  # noqa: F401  (re-exported to the test files)

f16, f32 = torch.float16, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDS = os.path.join(ROOT, "tests", "golden", "multi_control_records.safetensors")
# the seeded standard deviations of the site cases: with them the member's control share is far above 2 * TOL_Y of the output
# (checked on the CPU with the oracle alone: check_site_can_see_the_control_share)
UP_STD, CTRL_STD = 0.2, 1.0


# ------------------------------------------------------------------------------------------------ kernel
# (M, C, ldy, ranks of the members, rows_t as a divisor of M)
KERNEL_SHAPES = [
    (3 * 25, 72, 216, (4,), 1),
    (3 * 25, 72, 216, (4, 12, 16), 3),
    (2 * 64, 320, 960, (4, 8), 1),
    (2 * 64, 320, 320, (16,), 2),
    (2 * 16, 1280, 1280, (4,) * 8, 1),
    (2 * 16, 1280, 3840, (8, 8), 2),
    (3 * 128 + 3 * 7, 72, 216, (16, 16), 3),              # more than one 128-row chunk, a ragged last one
]


def mix_inputs(Mr, C, ldy, ranks, div, seed=0, dev="cpu"):
    """-> the [M, ldy] fp16 buffer whose first C columns are the q block, members [(T, toff, U, scale)], rows_t.  Each T sits at a
    column offset of a wider buffer, as the site's rank-space buffers do."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(Mr, ldy, generator=g).half().to(dev)
    rows_t = Mr // div
    members = []
    for i, r in enumerate(ranks):
        toff = 4 * (i % 3)
        T = torch.randn(rows_t, toff + r + 2, generator=g).to(dev)
        Uq = (torch.randn(C, r, generator=g) * 0.3).to(dev)
        members.append((T, toff, Uq, 0.49 if i % 2 == 0 else 1.0))
    return y, members, rows_t


def mix_reference(y, C, members, rows_t):
    """the update in fp64 (the scale as the fp32 value the kernel is handed), rounded to fp16 once"""
    ref = y[:, :C].double().cpu()
    reps = y.shape[0] // rows_t
    for T, toff, Uq, s in members:
        upd = T[:, toff:toff + Uq.shape[1]].double().cpu() @ Uq.double().cpu().t()
        ref = ref + float(torch.tensor(s, dtype=f32)) * upd.repeat(reps, 1)
    return ref.half()


def mix_reference_unrounded(y, C, members, rows_t):
    """-> (the update in fp64, unrounded;  the magnitude sum |Y| + sum |scale| |T| |U|^T that fp32 rounding errors scale with)"""
    ref = y[:, :C].double().cpu()
    mag = ref.abs()
    reps = y.shape[0] // rows_t
    for T, toff, Uq, s in members:
        t, u, sc = T[:, toff:toff + Uq.shape[1]].double().cpu(), Uq.double().cpu(), float(torch.tensor(s, dtype=f32))
        ref = ref + sc * (t @ u.t()).repeat(reps, 1)
        mag = mag + abs(sc) * (t.abs() @ u.abs().t()).repeat(reps, 1)
    return ref, mag


def check_mix_against_fp64(Mr, C, ldy, ranks, div, seed=0, dev="cpu", many_elements=False):
    """within 1 fp16 ulp of the fp64 evaluation rounded once; repeat launches bit-identical; columns past the q block untouched.
    many_elements (shapes with millions of elements, beyond the issue's list): among that many, some sums cancel to a result far
    below their terms, where the fp32 rounding of the terms (unit roundoff 2^-24 of magnitudes near 1) is no longer 'far inside
    half an fp16 ulp' of the tiny result.  There the 1-ulp limit is asserted wherever the terms' magnitude sum is at most 2^6
    times the result -- the fp32 error of the at most 32 products and the adds, (R + 2) 2^-24 mag <= 34 * 2^-18 |result|, is below
    a sixteenth of half an ulp -- and EVERY element is held to the fp32 error model: half an fp16 ulp plus (R + 2) 2^-24 mag."""
    y, members, rows_t = mix_inputs(Mr, C, ldy, ranks, div, seed, dev)
    y0 = y.clone()
    K.control_mix_q(y, C, members, rows_t)
    again = y0.clone()
    K.control_mix_q(again, C, members, rows_t)
    assert torch.equal(y, again), "a repeat launch is not bit-identical"
    ref = mix_reference(y0, C, members, rows_t)
    got = y[:, :C].contiguous()
    d = ulp_distance(got, ref)
    stats = dict(shape=(Mr, C, ldy), ranks=ranks, rows_t=rows_t, differ=float((d > 0).float().mean()), max_ulp=int(d.max()),
                 moved=float((ref != y0[:, :C].cpu()).float().mean()))
    if many_elements:
        ref64, mag = mix_reference_unrounded(y0, C, members, rows_t)
        plain = mag <= 64.0 * ref64.abs()
        stats["max_ulp"] = int(d[plain].max())
        stats["max_ulp_cancelling"] = int(d[~plain].max()) if bool((~plain).any()) else 0
        stats["cancelling"] = float((~plain).float().mean())
        big = torch.maximum(ref64.abs(), got.double().cpu().abs()).clamp_min(2.0 ** -14)
        half_ulp = 0.5 * torch.exp2(torch.floor(torch.log2(big)) - 10)
        excess = (got.double().cpu() - ref64).abs() - (half_ulp + (sum(ranks) + 2) * 2.0 ** -24 * mag)
        stats["worst_excess_over_fp32_model"] = float(excess.max())
    print("CONTROL_MIX_VS_FP64", stats)
    assert stats["max_ulp"] <= 1, stats
    if many_elements:
        assert stats["worst_excess_over_fp32_model"] <= 0.0, stats
    assert stats["moved"] > 0.5, ("the case must move the q block", stats)
    assert torch.equal(y[:, C:], y0[:, C:]), "columns past the q block were touched"
    return stats


def raw_job(y, C, members, rows_t, **override):
    """the C struct as kernels.control_mix_q builds it, with fields overridden: what the library itself must refuse"""
    job = capi.ControlMixJob(y.data_ptr(), y.stride(0), y.shape[0], C, rows_t, len(members))
    for i, (T, toff, Uq, s) in enumerate(members[:capi.CONTROL_MIX_MAX_MEMBERS]):
        job.m[i] = capi.ControlMixMember(T.data_ptr(), T.stride(0), toff, Uq.data_ptr(), Uq.stride(0), Uq.shape[1], float(s))
    for k, v in override.items():
        if k.startswith("m0_"):
            setattr(job.m[0], k[3:], v)
        else:
            setattr(job, k, v)
    return job


def check_contract_breaches(dev="cpu"):
    """every breach of the contract of include/clora.h returns ERR_ARG from the host and leaves Y as it was"""
    y, members, rows_t = mix_inputs(48, 72, 216, (4, 8), 2, seed=5, dev=dev)
    y0 = y.clone()
    lib = capi.lib().cdll
    wide = [(torch.randn(rows_t, 16).to(dev), 0, torch.randn(72, 16).to(dev), 1.0) for _ in range(3)]      # ranks sum to 48
    breaches = {
        "N % 8": raw_job(y, 68, members, rows_t),
        "ldy % 8": raw_job(y, 72, members, rows_t, ldy=212),
        "rank 0": raw_job(y, 72, members, rows_t, m0_r=0),
        "rank 17": raw_job(y, 72, members, rows_t, m0_r=17),
        "ranks sum to 48": raw_job(y, 72, wide, rows_t),
        "M % rows_t": raw_job(y, 72, members, 36),
        "no members": raw_job(y, 72, members, rows_t, nmem=0),
        "nine members": raw_job(y, 72, members, rows_t, nmem=9),
    }
    for what, job in breaches.items():
        rc = lib.clora_control_mix_q_f16(ctypes.byref(job), capi.stream())
        assert rc == capi.ERR_ARG, (what, rc)
    if dev != "cpu":
        torch.cuda.synchronize()
    assert torch.equal(y, y0), "a refused job wrote to Y"
    assert lib.clora_control_mix_q_f16(ctypes.byref(raw_job(y, 72, members, rows_t)), capi.stream()) == capi.OK
    assert not torch.equal(y, y0)


# ------------------------------------------------------------------------------------------------ one site
ARRANGEMENTS = ("control_pre", "control_post_plain_pre", "two_control")


def _seeded(o, seed, up_std=UP_STD):
    cases.seeded_weights_(o, seed=seed, up_std=up_std)
    return o


def _control_pair(C, cad, rank, seed, dev, skip=None, cls="v1", ctrl_c=None, **kw):
    """a control processor in oracle and product form with the same seeded weights"""
    if cls == "v1":
        o, p = cr.ControlLoRAProcRef(C, cad, rank=rank, **kw), M.ControlLoRACrossAttnProcessor(C, cad, rank=rank, **kw)
    else:
        o = cr.ControlLoRAProcV2Ref(C, cad, rank=rank, control_channels=ctrl_c)
        p = M.ControlLoRACrossAttnProcessorV2(C, cad, rank=rank, control_channels=ctrl_c)
    _seeded(o, seed)
    p.load_state_dict(o.state_dict())
    p.to(dev)
    if skip == "value":
        o.skip_value_states(True)
        p.skip_value_states(True)
    return o, p


def _plain_pair(C, cad, rank, seed, dev):
    o, p = cr.LoRAProcRef(C, cad, rank=rank), M.LoRACrossAttnProcessor(C, cad, rank=rank)
    _seeded(o, seed)
    p.load_state_dict(o.state_dict())
    p.to(dev)
    return o, p


def _attn_pair(C, cad, heads, dev):
    o_attn = unet_ref.CrossAttention(C, cad, heads=heads, dim_head=C // heads)
    cases.seeded_weights_(o_attn, seed=5)
    p_attn = U.CrossAttention(C, cad, heads=heads, dim_head=C // heads)
    with torch.no_grad():
        for k, v in p_attn.state_dict().items():
            v.copy_(o_attn.state_dict()[k].to(v.dtype))
        for q in o_attn.parameters():                      # oracle: fp32 math on fp16-rounded frozen weights
            q.data = q.data.half().float()
    return o_attn, p_attn.to(dev)


def build_site(self_attn, arrangement, dev, C=64, heads=4, ctx=48, B=2, side=4, ctrl_batch=None, seed=0, main="v1", member_kw=None):
    """a main control processor with control members chained on.  Every control processor has a control map of its own;
    ctrl_batch: the members' control batch (default B; 1 = one map for the whole batch)"""
    g = torch.Generator().manual_seed(seed)
    N = side * side
    cad = None if self_attn else ctx
    o_attn, p_attn = _attn_pair(C, cad, heads, dev)
    if main == "v1":
        o_main, p_main = _control_pair(C, cad, 4, 1, dev)
    else:
        o_main, p_main = _control_pair(C, cad, 4, 1, dev, cls="v2", ctrl_c=C)
    member_kw = member_kw or {}
    Ca = _control_pair(C, cad, 4, 2, dev, **member_kw)
    Cb = _control_pair(C, cad, 4, 3, dev, skip="value")
    Pl = _plain_pair(C, cad, 8, 4, dev)
    pre, post = {"control_pre": ([Ca], []), "control_post_plain_pre": ([Pl], [Ca]), "two_control": ([Ca], [Cb])}[arrangement]
    for o, p in pre:
        o_main.inject_pre_lora(o); p_main.inject_pre_lora(p)
    for o, p in post:
        o_main.inject_post_lora(o); p_main.inject_post_lora(p)
    h = torch.randn(B, N, C, generator=g).half()
    e = None if self_attn else torch.randn(B, 5, ctx, generator=g).half()
    cb = B if ctrl_batch is None else ctrl_batch
    ctrl = torch.randn(B, C, side, side, generator=g).half() * CTRL_STD
    member_ctrl = {id(o): torch.randn(cb, C, side, side, generator=g).half() * CTRL_STD for o, _ in (Ca, Cb)}
    s = dict(o_attn=o_attn, p_attn=p_attn, o_main=o_main, p_main=p_main, h=h, e=e, ctrl=ctrl, B=B, N=N, dev=dev,
             members=pre + post, member_ctrl=member_ctrl)
    inject_member_controls(s)
    return s


def tokens(ctrl, dev):
    b, c, hh, ww = ctrl.shape
    return ctrl.permute(0, 2, 3, 1).reshape(b, hh * ww, c).contiguous().to(dev)


def inject_member_controls(s, scale_by=1.0):
    """every control member's own map into its oracle and product processor (fresh tensors: what a new guide does)"""
    for o, p in s["members"]:
        c = s["member_ctrl"].get(id(o))
        if c is not None:
            c = (c.float() * scale_by).half()
            o.inject_control_states(c.float())
            p.inject_control_states(tokens(c, s["dev"]))


def oracle_site(s, o_main=None):
    o_main = s["o_main"] if o_main is None else o_main
    o_main.inject_control_states(s["ctrl"].float())
    with torch.no_grad():
        return o_main(s["o_attn"], s["h"].float(), None if s["e"] is None else s["e"].float(), None, SCALE)


def product_site(s, p_main=None, scale=SCALE, grad=False, fused=None):
    """fused: None = the switches as they are; True / False sets fold_chain and fold_control_members"""
    p_main = s["p_main"] if p_main is None else p_main
    if fused is not None:
        p_main.fold_chain = p_main.fold_control_members = bool(fused)
    dev = s["dev"]
    p_main.inject_control_states(tokens(s["ctrl"], dev))
    e = None if s["e"] is None else s["e"].to(dev)
    with torch.set_grad_enabled(grad):
        return p_main(s["p_attn"], s["h"].clone().to(dev), e, None, scale)


def broken_oracles(s):
    """the oracle chain with the members' control share broken, as deep copies of the oracle processors:
    'no_control': every member's control states zeroed;  's_not_s2': every member's share s^2 U_q t scaled by s instead, i.e.
    the member's control term evaluated at scale 1 (its `to_control.up` divided by the call's scale)"""
    out = {}
    o = copy.deepcopy(s["o_main"])
    for m in o.pre_loras + o.post_loras:
        if isinstance(m, cr.ControlLoRAProcRef):
            m.inject_control_states(torch.zeros_like(m.control_states))
    out["no_control"] = o
    o = copy.deepcopy(s["o_main"])
    with torch.no_grad():
        for m in o.pre_loras + o.post_loras:
            if isinstance(m, cr.ControlLoRAProcRef):
                m.to_control.up.weight.div_(SCALE)
    out["s_not_s2"] = o
    return out


def check_site_can_see_the_control_share(s, tag):
    yo = oracle_site(s)
    wrong = {k: rel(oracle_site(s, o), yo) for k, o in broken_oracles(s).items()}
    print(f"MULTI_CONTROL_SITE {tag}: oracle with the members' control share broken sits", {k: f"{v:.3e}" for k, v in wrong.items()}, "away")
    for k, v in wrong.items():
        assert v > 2 * TOL_Y, (tag, k, v, "the case cannot see the control share")
    return yo


def check_fused_site(arrangement, dev, **shape):
    """fused site vs the oracle chain, no autograd; the generic path's error beside it"""
    worst = {}
    for self_attn in (True, False):
        s = build_site(self_attn, arrangement, dev, **shape)
        tag = f"{arrangement}/{'self' if self_attn else 'cross'}"
        yo = check_site_can_see_the_control_share(s, tag)
        with torch.no_grad():
            y_gen = product_site(s, fused=False)
            assert "_fold" not in s["p_main"].__dict__ and "_mix" not in s["p_main"].__dict__
            y_fused = product_site(s, fused=True)
            assert s["p_main"]._fold_blocker() is None and not s["p_main"]._needs_generic_path(), s["p_main"]._fold_blocker()
            assert "_fold" in s["p_main"].__dict__ and "_mix" in s["p_main"].__dict__
        e_fused, e_gen = rel(y_fused, yo), rel(y_gen, yo)
        print(f"MULTI_CONTROL_SITE {tag}: fused {e_fused:.3e}  generic {e_gen:.3e}  (limit {TOL_Y})")
        assert e_fused < TOL_Y, (tag, e_fused)
        worst[tag] = (e_fused, e_gen)
    return worst


# ------------------------------------------------------------------------------------------------ reference records
def load_records():
    """-> {"<case>:<self|cross>:cb<control batch>": dict(attn.*, main.*, member<i>.*, h, e, ctrl.main, ctrl.member<i>, y)}.  The file
    stores what records share once: the two attention modules, h, e, and a case's processor weights for both control batches."""
    from safetensors.torch import load_file
    flat = load_file(RECORDS)
    recs = {}
    for k, v in flat.items():
        head, name = k.split("/", 1)
        if head.count(":") == 2:
            recs.setdefault(head, {})[name] = v
    for name, rec in recs.items():
        case, where, _ = name.split(":")
        for k, v in flat.items():
            head, sub = k.split("/", 1)
            if head == f"attn.{where}":
                rec["attn." + sub] = v
            elif head == f"w.{case}:{where}":
                rec[sub] = v
        rec["h"] = flat["shared/h"]
        if where == "cross":
            rec["e"] = flat["shared/e"]
    return recs


RECORD_CASES = ("v1.control_pre", "v1.control_post_plain_pre", "v1.two_control", "v2.member_pre", "v2.member_post")
GEOM = dict(C=64, heads=4, ctx=48, N=16, B=2, scale=0.7, ctrl_c_v2=32)


def record_chain(case, self_attn, mods):
    """the processors of one recorded case, built from `mods` = dict(attn=, control=, control_v2=, plain=) of constructors (the
    reference's classes when the records are written, the oracle's or the product's when they are read) -> (main, [members])"""
    C, ctx = GEOM["C"], GEOM["ctx"]
    cad = None if self_attn else ctx
    if case.startswith("v1"):
        main = mods["control"](C, cad, rank=4)
        a = mods["control"](C, cad, rank=4)
        if case == "v1.control_pre":
            main.inject_pre_lora(a)
            return main, [a]
        if case == "v1.control_post_plain_pre":
            pl = mods["plain"](C, cad, rank=8)
            main.inject_pre_lora(pl)
            main.inject_post_lora(a)
            return main, [pl, a]
        b = mods["control"](C, cad, rank=4)
        b.skip_value_states(True)
        main.inject_pre_lora(a)
        main.inject_post_lora(b)
        return main, [a, b]
    main = mods["control_v2"](C, cad, rank=4, control_channels=GEOM["ctrl_c_v2"])
    a = mods["control_v2"](C, cad, rank=4, control_channels=GEOM["ctrl_c_v2"])
    (main.inject_pre_lora if case == "v2.member_pre" else main.inject_post_lora)(a)
    return main, [a]


def _load_prefixed(module, rec, prefix):
    sd = {k[len(prefix):]: v for k, v in rec.items() if k.startswith(prefix)}
    module.load_state_dict({k: v.to(module.state_dict()[k].dtype) for k, v in sd.items()})


def replay_record(name, rec, side, dev="cpu"):
    """one record through the oracle ('oracle', fp32 on the recorded weights) or the product's generic path ('product')
    -> (y, recorded y)"""
    case, where, _ = name.split(":")
    self_attn = where == "self"
    C, heads, ctx = GEOM["C"], GEOM["heads"], GEOM["ctx"]
    cad = None if self_attn else ctx
    if side == "oracle":
        mods = dict(control=cr.ControlLoRAProcRef, control_v2=cr.ControlLoRAProcV2Ref, plain=cr.LoRAProcRef)
        attn = unet_ref.CrossAttention(C, cad, heads=heads, dim_head=C // heads)
    else:
        mods = dict(control=M.ControlLoRACrossAttnProcessor, control_v2=M.ControlLoRACrossAttnProcessorV2, plain=M.LoRACrossAttnProcessor)
        attn = U.CrossAttention(C, cad, heads=heads, dim_head=C // heads)
    main, members = record_chain(case, self_attn, mods)
    _load_prefixed(attn, rec, "attn.")
    _load_prefixed(main, rec, "main.")
    for i, m in enumerate(members):
        _load_prefixed(m, rec, f"member{i}.")
    h, e = rec["h"], rec.get("e")
    if side == "oracle":
        main.inject_control_states(rec["ctrl.main"].float())
        for i, m in enumerate(members):
            if f"ctrl.member{i}" in rec:
                m.inject_control_states(rec[f"ctrl.member{i}"].float())
        with torch.no_grad():
            y = main(attn, h.float(), None if e is None else e.float(), None, GEOM["scale"])
    else:
        attn.to(dev); main.to(dev)
        main.inject_control_states(tokens(rec["ctrl.main"].half(), dev))
        for i, m in enumerate(members):
            m.to(dev)
            if f"ctrl.member{i}" in rec:
                m.inject_control_states(tokens(rec[f"ctrl.member{i}"].half(), dev))
        with torch.no_grad():
            y = main(attn, h.half().to(dev), None if e is None else e.half().to(dev), None, GEOM["scale"])
    return y, rec["y"]


# ------------------------------------------------------------------------------------------------ whole small UNets
def seeded_control_pair(case, dev, seed, up_std=0.05):
    """a second (third ...) control model for the small topology in oracle and product form, with seeded non-zero weights"""
    torch.manual_seed(seed)
    o = cr.ControlLoRARef(**cases.CASES[case])
    with torch.no_grad():
        g = torch.Generator().manual_seed(seed)
        for n, q in o.named_parameters():
            if ".up.weight" in n:
                q.copy_(torch.randn(q.shape, generator=g) * up_std)
    p = M.ControlLoRA(**cases.CASES[case])
    p.load_state_dict(o.state_dict())
    return o, p.to(dev)


def mix_oracle_controls(o_unet, o_main, o_members, pre=True, post=False):
    sites = cr.map_processors_to_unet(o_unet, o_main)
    for i, om in enumerate(o_members):
        msites = cr.map_processors_to_unet(o_unet, om)
        for name, proc in sites.items():
            if pre:
                proc.inject_pre_lora(msites[name])
            if post:
                proc.inject_post_lora(msites[name])
            proc.add_module(f"mixed_control_member{i}", msites[name])
    o_unet.set_attn_processor(sites)


def two_control_small_pair(dev, fold=True, case="v1"):
    """small topology steered by two control models, mixed identically in oracle and product
    -> (o_unet, [o_main, o_member], p_unet, [p_main, p_member])"""
    from tests.e2e_cases import build_product_case
    o_unet, _, o_main = cases.build_oracle_case(case)
    p_unet, _, p_main = build_product_case(case, dev)
    with torch.no_grad():
        for q in o_unet.parameters():                      # frozen weights: fp16 values on both sides
            q.copy_(q.half().float())
    o_mem, p_mem = seeded_control_pair(case, dev, seed=41)
    mix_oracle_controls(o_unet, o_main, [o_mem])
    M.mix_control_loras(p_unet, p_main, [p_mem], pre=True, post=False, fold=fold)
    return o_unet, [o_main, o_mem], p_unet, [p_main, p_mem]


def small_inputs():
    """the seeded inputs cut down to a 64 x 64 guide and 8 x 8 latents: every level of the small topology still has tokens"""
    inp = cases.seeded_inputs()
    return dict(inp, guide=inp["guide"][:, :, :64, :64].contiguous(), latents=inp["latents"][:, :, :8, :8].contiguous())


def forward(unet, cloras, inp, guides, dev):
    with torch.no_grad():
        for c, gd in reversed(list(zip(cloras, guides))):  # members first: the main model's forward sees a chain that folds
            c(gd[:1].half().to(dev))
        return unet(inp["latents"].half().to(dev), 501, inp["ehs"].half().to(dev)).sample


def check_two_control_unet(dev):
    """one forward of the small topology under two control models: fused and generic against the oracle chain, and the library
    calls of the fused forward = the single-control forward's + the member's hint encoder + exactly one per site"""
    from tests.e2e_cases import build_product_case
    inp = small_inputs()
    g = torch.Generator().manual_seed(9)
    guides = [inp["guide"], torch.rand(inp["guide"].shape, generator=g) * 2 - 1]
    o_unet, o_cl, p_unet, p_cl = two_control_small_pair(dev, fold=True)
    with torch.no_grad():
        for oc, gd in zip(o_cl, guides):
            oc(gd[:1])
        yo = o_unet(inp["latents"], 501, inp["ehs"]).sample
    single_unet, _, single = build_product_case("v1", dev)
    forward(single_unet, [single], inp, guides[:1], dev)
    with count_library_calls() as names:
        y_single = forward(single_unet, [single], inp, guides[:1], dev)
    n_single = len(names)
    forward(p_unet, p_cl, inp, guides, dev)                 # warm: lazy packs, the fold, the jobs
    with torch.no_grad():
        rep = p_cl[0].fold_report()
    assert all(r["folded"] and r["control_members"] == 1 for r in rep.values()), rep
    with count_library_calls() as names:
        y_fused = forward(p_unet, p_cl, inp, guides, dev)
    with count_library_calls() as hint:
        with torch.no_grad():
            p_cl[1](guides[1][:1].half().to(dev))
    n_hint = len(hint)
    sites = len(p_unet.attn_processors)
    print(f"LAUNCHES small topology: single control {n_single}, two controls fused {len(names)} "
          f"(of them the member's hint encoder {n_hint}), sites {sites}")
    assert names.count("clora_control_mix_q_f16") == sites
    assert "clora_lora_fold_f16" not in names
    # beyond the member's own hint encoder (with its rank-space terms, which the jobs reuse): one launch per site
    assert len(names) - n_hint == n_single + sites, (len(names), n_hint, n_single, sites)
    p_cl[0].fold_chains(False)
    y_gen = forward(p_unet, p_cl, inp, guides, dev)
    e_fused, e_gen = rel(y_fused, yo), rel(y_gen, yo)
    print(f"TWO_CONTROL small UNet forward vs oracle chain: fused {e_fused:.3e}  generic {e_gen:.3e};  "
          f"second control moves the output by {rel(y_fused, y_single):.3e}")
    assert rel(y_fused, y_single) > 10 * e_fused, "the second control model must matter"
    assert e_fused < 5.5e-3 and e_gen < 5.5e-3, (e_fused, e_gen)


def check_sampler_lists(dev, **kw):
    """ddim_sample with lists: a list of one is the single call bit for bit; two models fused agree with two models generic"""
    import pytest
    from controllora_amd.pipeline import ddim_sample
    from tests.e2e_cases import build_product_case
    inp = small_inputs()
    unet, _, clora = build_product_case("v1", dev)
    cond, uncond = inp["ehs"][:1].half().to(dev), inp["ehs"][1:2].half().to(dev)
    guide = inp["guide"][:1].half().to(dev)
    kw = dict(dict(steps=1, guidance_scale=3.0, graph=False), **kw)
    lat = inp["latents"][:1].half().to(dev)
    a = ddim_sample(unet, clora, guide, cond, uncond, latents=lat.clone(), **kw)
    b = ddim_sample(unet, [clora], [guide], cond, uncond, latents=lat.clone(), **kw)
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="guide"):
        ddim_sample(unet, [clora], [guide, guide], cond, uncond, latents=lat.clone(), **kw)
    _, member = seeded_control_pair("v1", dev, seed=41)
    M.mix_control_loras(unet, clora, [member], fold=True)
    g2 = (torch.rand(guide.shape, generator=torch.Generator().manual_seed(3)) * 2 - 1).half().to(dev)
    c = ddim_sample(unet, [clora, member], [guide, g2], cond, uncond, latents=lat.clone(), **kw)
    with torch.no_grad():
        assert all(r["folded"] for r in clora.fold_report().values())
    clora.fold_chains(False)
    d = ddim_sample(unet, [clora, member], [guide, g2], cond, uncond, latents=lat.clone(), **kw)
    assert not torch.equal(c, a) and rel(c, d) < 5.5e-3 < rel(c, a), (rel(c, d), rel(c, a))


# ---- sampler parity against the oracle loop, at the settings of tests/test_lora_fold_gpu.test_mixed_folded_ddim_small_50_steps
class _OracleControls:
    """the hint encoders of several oracle control models behind the one-model call of tests.full_cases.oracle_ddim"""

    def __init__(self, models, guides):
        self.models, self.guides = models, guides

    def __call__(self, _guide):
        for m, gd in zip(self.models, self.guides):
            m(gd.to(next(m.parameters()).dtype).to(next(m.parameters()).device))


_SAMPLER_ORACLE = {}


def two_control_sampler_case(dev, res=128, steps=50, guidance_scale=9.0, nb=2, ctx_dim=64, ctx_len=7, seed=5):
    """-> dict(inputs, the fp32 oracle's latents, the fp16-regime oracle's distance from them): computed once per process"""
    from tests import full_cases as F
    if "case" in _SAMPLER_ORACLE:
        return _SAMPLER_ORACLE["case"]
    g = torch.Generator().manual_seed(seed)
    L = res // 8
    guides = [((torch.rand(1, 3, res, res, generator=g) > 0.9).float() * 2 - 1) for _ in range(2)]
    cond = torch.randn(nb, ctx_len, ctx_dim, generator=g).half().float()
    uncond = torch.randn(nb, ctx_len, ctx_dim, generator=g).half().float()
    lat0 = torch.randn(nb, 4, L, L, generator=g).half().float()
    o_unet, o_cl, _, _ = pair = two_control_small_pair(dev, fold=True)
    with torch.no_grad():
        ref, _ = F.oracle_ddim(o_unet, _OracleControls(o_cl, guides), None, cond, uncond, steps, guidance_scale, lat0)

        def low_precision(where):
            """the same loop with every module and tensor in fp16 (tests.full_cases.fp16_oracle_floor, for several control models)"""
            h_unet, h_cl = copy.deepcopy((o_unet, o_cl))
            h_unet.half().to(where)
            for m in h_cl:
                m.half().to(where)
            mv = lambda t: t.half().to(where)
            out, _ = F.oracle_ddim(h_unet, _OracleControls(h_cl, guides), None, mv(cond), mv(uncond), steps, guidance_scale, mv(lat0))
            return out.float().cpu()

        try:
            low = low_precision(dev)
        except RuntimeError as e:                           # an oracle module that builds a tensor on the host: the host loop instead
            print("NOTE two_control_sampler_case: the fp16 oracle failed on", dev, "->", str(e).splitlines()[0][:200])
            low = low_precision("cpu")
    case = dict(guides=guides, cond=cond, uncond=uncond, lat0=lat0, ref=ref, floor=rel(low, ref), steps=steps,
                guidance_scale=guidance_scale, pair=pair)
    _SAMPLER_ORACLE["case"] = case
    return case


def two_control_sample(case, dev, fused, graph):
    from controllora_amd.pipeline import ddim_sample
    _, _, p_unet, p_cl = case["pair"]
    p_cl[0].fold_chains(bool(fused), control_members=bool(fused))
    mv = lambda t: t.to(dev).half()
    out = ddim_sample(p_unet, p_cl, [mv(gd) for gd in case["guides"]], mv(case["cond"]), mv(case["uncond"]), steps=case["steps"],
                      guidance_scale=case["guidance_scale"], latents=mv(case["lat0"]), graph=graph)
    with torch.no_grad():
        rep = p_cl[0].fold_report()
    assert all(r["folded"] == bool(fused) for r in rep.values()), rep
    return out
