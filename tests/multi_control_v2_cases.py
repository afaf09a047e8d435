"""Shared cases of the chained version-2 ControlLoRA tests (CPU on the emulated kernels, GPU on the real library): the control-chain
kernel (clora_control_chain_f16) against an fp64 evaluation of its three formulas, one v2 attention site with frozen v2 control members
chained on against the oracle's chain (oracle/controllora_ref.py), the recorded reference outputs of the v2 chains
(tests/golden/multi_control_records.safetensors) through the fused path, and whole small UNets steered by two v2 control models."""
import copy
import ctypes
import types

import torch

from controllora_amd import capi, kernels as K, models as M
from oracle import cases, controllora_ref as cr
from tests import multi_control_cases as MC
from tests.e2e_cases import rel
from tests.lora_fold_cases import SCALE, TOL_Y, count_library_calls, ulp_distance  # noqa: F401  (re-exported to the test files)

f16, f32 = torch.float16, torch.float32
# the seeded standard deviations of the site cases.  The coupling between the processors of a chain is second order in the up
# matrices (s^2 U_i Dh_i U_j t_j): with these the oracle chain sits far more than 2 * TOL_Y away from the chain without coupling,
# without the members' control maps and with the order swapped (checked on the CPU with the oracle alone: check_site_can_see)
UP_STD, CTRL_STD = 0.5, 1.0
UNET_LIMIT = 5.5e-3          # the limit of multi_control_cases.check_two_control_unet (v1)


# ------------------------------------------------------------------------------------------------ kernel
# (M, C, ranks of the members, rows_t as a divisor of M)
KERNEL_SHAPES = [
    (75, 72, (4,), 1),                          # C no multiple of 64
    (75, 72, (4, 12, 16), 3),                   # R = 32, a broadcast control map
    (128, 320, (4, 4), 1),
    (32, 1280, (4,) * 8, 1),                    # eight members, the widest C
    (32, 1280, (16, 16), 2),
    (3 * 128 + 21, 72, (8, 8), 3),              # several row chunks, a ragged last one
]


def chain_inputs(Mr, C, ranks, div, seed=0, dev="cpu", padded=False):
    """-> H [M, C] fp16 (a view of a wider buffer when padded), members [(Dh, U, Tc, toff)], G, rows_t.  Magnitudes of a trained
    model: down rows of unit response (p ~ 1), up matrices N(0, 0.02) as in lora_fold_cases.fold_inputs -- the update then moves
    most elements by many fp16 steps, while its fp32 rounding error (about 1e-8) stays below the smallest fp16 step everywhere, zero
    crossings of the result included.  Dh is the first C columns of a [r, C + Cc] down matrix (ldd > C when padded).  The blocks of G
    on and above the block diagonal hold NaN: the kernel must not read them."""
    g = torch.Generator().manual_seed(seed)
    ldh = C + 8 if padded else C
    H = torch.randn(Mr, ldh, generator=g).half().to(dev)[:, :C]
    rows_t = Mr // div
    R = sum(ranks)
    G = torch.full((R, R), float("nan"))
    members, off = [], 0
    for i, r in enumerate(ranks):
        Cc = 12 if padded else 0
        toff = 4 * ((i + 1) % 3) if padded else 0
        D = (torch.randn(r, C + Cc, generator=g) / C ** 0.5).to(dev)
        Uw = (torch.randn(C, r, generator=g) * 0.02).to(dev)
        Tc = torch.randn(rows_t, toff + r + 2, generator=g).to(dev)
        G[off:off + r, :off] = torch.randn(r, off, generator=g) * 0.1
        members.append((D[:, :C], Uw, Tc, toff))
        off += r
    return H, members, G.to(dev), rows_t


def chain_reference(H, members, G, s, rows_t, coupled=True):
    """the three formulas of include/clora.h in fp64 (the scale as the fp32 value the kernel is handed), rounded to fp16 once;
    evaluated where the inputs live"""
    Hd = H.double()
    reps = H.shape[0] // rows_t
    s = float(torch.tensor(s, dtype=f32))
    Gd = G.double()
    ts, off = [], 0
    upd = torch.zeros_like(Hd)
    for Dh, Uw, Tc, toff in members:
        r = Uw.shape[1]
        t = Hd @ Dh.double().t() + Tc[:, toff:toff + r].double().repeat(reps, 1)
        if coupled:
            for tj, oj in ts:
                t = t + s * tj @ Gd[off:off + r, oj:oj + tj.shape[1]].t()
        ts.append((t, off))
        upd = upd + t @ Uw.double().t()
        off += r
    return (Hd + s * upd).half().cpu()


def check_chain_against_fp64(Mr, C, ranks, div, seed=0, dev="cpu", in_place=False, padded=False, scale=SCALE):
    """every element within 1 fp16 ulp of the fp64 evaluation rounded once; a repeat launch bit-identical; H left alone (or, in
    place, replaced); columns of a padded output past C untouched"""
    H, members, G, rows_t = chain_inputs(Mr, C, ranks, div, seed, dev, padded)
    H0 = H.clone()
    ref = chain_reference(H0, members, G, scale, rows_t)

    def run():
        h = torch.zeros(Mr, C + 8 if padded else C, dtype=f16, device=dev)[:, :C]
        h.copy_(H0)
        if in_place:
            return K.control_chain(h, h, members, G, scale, rows_t), h
        ybuf = torch.full((Mr, C + 16 if padded else C), 3.0, dtype=f16, device=dev)
        y = K.control_chain(h, ybuf[:, :C], members, G, scale, rows_t)
        assert torch.equal(h, H0), "the input was written"
        if padded:
            assert bool((ybuf[:, C:] == 3.0).all()), "columns past C were touched"
        return y, h

    y, _ = run()
    again, _ = run()
    assert torch.equal(y, again), "a repeat launch is not bit-identical"
    got = y.contiguous()
    d = ulp_distance(got, ref)
    loose = chain_reference(H0, members, G, scale, rows_t, coupled=False)
    stats = dict(shape=(Mr, C), ranks=ranks, rows_t=rows_t, in_place=in_place, padded=padded, differ=float((d > 0).float().mean()),
                 max_ulp=int(d.max()), moved=float((ref != H0.cpu()).float().mean()),
                 coupling_seen=float((ulp_distance(loose, ref) > 1).float().mean()))
    print("CONTROL_CHAIN_VS_FP64", stats)
    assert bool(torch.isfinite(got.float()).all()), "a block of G on or above the block diagonal was read"
    assert stats["max_ulp"] <= 1, stats
    assert stats["moved"] > 0.5, ("the case must move the hidden states", stats)
    if len(ranks) > 1:
        assert stats["coupling_seen"] > 0.25, ("the case must see the coupling through G", stats)
    return stats


def raw_job(h, y, members, G, scale, rows_t, **override):
    """the C struct as kernels.control_chain builds it, with fields overridden: what the library itself must refuse"""
    job = K.control_chain_job(h, y, members, G, scale, rows_t)
    for k, v in override.items():
        if k.startswith("m0_"):
            setattr(job.m[0], k[3:], v)
        elif k.startswith("job_"):
            setattr(job, k[4:], v)
        else:
            setattr(job, k, v)
    return job


def check_contract_breaches(dev="cpu"):
    """every breach of the contract of include/clora.h returns ERR_ARG from the host and leaves Y as it was"""
    H, members, G, rows_t = chain_inputs(48, 72, (4, 8), 2, seed=5, dev=dev)
    buf = torch.randn(48 + 8, 72, generator=torch.Generator().manual_seed(6)).half().to(dev)
    y = buf[8:]
    buf0 = buf.clone()
    lib = capi.lib().cdll
    g = torch.Generator().manual_seed(7)
    wide = [((torch.randn(r, 72, generator=g) / 8).to(dev), (torch.randn(72, r, generator=g) * 0.02).to(dev),
             torch.randn(rows_t, r, generator=g).to(dev), 0) for r in (16, 16, 1)]                    # ranks sum to 33
    Gw = torch.zeros(33, 33).to(dev)
    narrow = [(m[0][:, :64], m[1][:64], m[2], m[3]) for m in members]
    breaches = {
        "rank 17": raw_job(H, y, members, G, SCALE, rows_t, m0_r=17),
        "rank 0": raw_job(H, y, members, G, SCALE, rows_t, m0_r=0),
        "ranks sum to 33": raw_job(H, y, wide, Gw, SCALE, rows_t),
        "no members": raw_job(H, y, members, G, SCALE, rows_t, nmem=0),
        "nine members": raw_job(H, y, members, G, SCALE, rows_t, nmem=9),
        "C % 8": raw_job(H[:, :64], y[:, :64], narrow, G, SCALE, rows_t, C=68),
        "ldh % 8": raw_job(H, y, members, G, SCALE, rows_t, ldh=76),
        "ldy < C": raw_job(H, y, members, G, SCALE, rows_t, ldy=64),
        "M % rows_t": raw_job(H, y, members, G, SCALE, rows_t, job_rows_t=36),
        "partial overlap": raw_job(buf[:48], y, members, G, SCALE, rows_t),
        "the same rows at another pitch": raw_job(y, y, members, G, SCALE, rows_t, ldh=144),
    }
    for what, job in breaches.items():
        rc = lib.clora_control_chain_f16(ctypes.byref(job), capi.stream())
        assert rc == capi.ERR_ARG, (what, rc)
    if dev != "cpu":
        torch.cuda.synchronize()
    assert torch.equal(buf, buf0), "a refused job wrote to Y"
    assert lib.clora_control_chain_f16(ctypes.byref(raw_job(H, y, members, G, SCALE, rows_t)), capi.stream()) == capi.OK
    assert not torch.equal(buf[8:], buf0[8:]) and torch.equal(buf[:8], buf0[:8])


# ------------------------------------------------------------------------------------------------ one site
ARRANGEMENTS = ("member_pre", "member_post", "plain_pre_member_post", "two_members", "member_batch_1")
MAIN_CTRL_C = 32


def _v2_pair(C, cad, rank, seed, dev, ctrl_c, up_std=UP_STD):
    o, p = MC._control_pair(C, cad, rank, seed, "cpu", cls="v2", ctrl_c=ctrl_c)
    cases.seeded_weights_(o, seed=seed, up_std=up_std)
    p.load_state_dict(o.state_dict())
    return o, p.to(dev)


def build_site(self_attn, arrangement, dev, C=64, heads=4, ctx=48, B=2, side=4, seed=0, member_rank=4, n_members=8):
    """a v2 main control processor with v2 control members (and a plain LoRA) chained on; every control processor has a control map
    of its own, the two members of 'two_members' over different channel counts.  Same dict as multi_control_cases.build_site."""
    g = torch.Generator().manual_seed(seed)
    N = side * side
    cad = None if self_attn else ctx
    o_attn, p_attn = MC._attn_pair(C, cad, heads, dev)
    o_main, p_main = _v2_pair(C, cad, 4, 1, dev, MAIN_CTRL_C)
    Ca = _v2_pair(C, cad, member_rank, 2, dev, 48)
    Cb = _v2_pair(C, cad, 4, 3, dev, 16)
    Pl = MC._plain_pair(C, cad, 8, 4, dev)
    if arrangement == "many_members":
        many = [_v2_pair(C, cad, 2, 10 + i, dev, 16) for i in range(n_members)]
        pre, post = many[:n_members // 2], many[n_members // 2:]
    else:
        many = []
        pre, post = {"member_pre": ([Ca], []), "member_post": ([], [Ca]), "plain_pre_member_post": ([Pl], [Ca]),
                     "two_members": ([Ca], [Cb]), "member_batch_1": ([Ca], [Cb])}[arrangement]
    for o, p in pre:
        o_main.inject_pre_lora(o); p_main.inject_pre_lora(p)
    for o, p in post:
        o_main.inject_post_lora(o); p_main.inject_post_lora(p)
    h = torch.randn(B, N, C, generator=g).half()
    e = None if self_attn else torch.randn(B, 5, ctx, generator=g).half()
    cb = 1 if arrangement == "member_batch_1" else B
    ctrl = torch.randn(B, MAIN_CTRL_C, side, side, generator=g).half() * CTRL_STD
    member_ctrl = {id(o): torch.randn(cb, o.to_control.down.weight.shape[1] - C, side, side, generator=g).half() * CTRL_STD
                   for o, _ in [Ca, Cb] + many}
    s = dict(o_attn=o_attn, p_attn=p_attn, o_main=o_main, p_main=p_main, h=h, e=e, ctrl=ctrl, B=B, N=N, dev=dev,
             members=pre + post, member_ctrl=member_ctrl)
    MC.inject_member_controls(s)
    return s


def broken_oracles(s):
    """the oracle chain broken in the three ways a wrong fused chain would be, as deep copies of the oracle processors:
    'no_coupling': every v2 processor reads the ORIGINAL hidden states (G = 0);  'no_member_control': the members' control maps
    zeroed;  'order_swapped': the pre and the post members exchanged (a lone member then changes sides of the main processor)"""
    out = {}
    o = copy.deepcopy(s["o_main"])

    def uncoupled(is_out):
        def f(self, x, scale):
            y = x
            for p in self._chain():
                if isinstance(p, cr.ControlLoRAProcV2Ref):
                    y = y + p.process_control_states(x, scale, is_out=is_out)
            return y
        return f
    o._pre = types.MethodType(uncoupled(False), o)
    o._post_attn = types.MethodType(uncoupled(True), o)
    out["no_coupling"] = o
    o = copy.deepcopy(s["o_main"])
    for m in o.pre_loras + o.post_loras:
        if isinstance(m, cr.ControlLoRAProcV2Ref):
            m.inject_control_states(torch.zeros_like(m.control_states))
    out["no_member_control"] = o
    o = copy.deepcopy(s["o_main"])
    o.pre_loras, o.post_loras = o.post_loras, o.pre_loras
    out["order_swapped"] = o
    return out


def check_site_can_see(s, tag):
    yo = MC.oracle_site(s)
    wrong = {k: rel(MC.oracle_site(s, o), yo) for k, o in broken_oracles(s).items()}
    print(f"MULTI_CONTROL_V2_SITE {tag}: the oracle chain broken sits", {k: f"{v:.3e}" for k, v in wrong.items()}, f"away (2 TOL_Y = {2 * TOL_Y})")
    for k, v in wrong.items():
        assert v > 2 * TOL_Y, (tag, k, v, "the case cannot see what the fused chain adds")
    return yo


def states(p):
    return sorted(k for k in ("_fold", "_mix", "_chain") if k in p.__dict__)


def check_fused_site(arrangement, dev, **shape):
    """fused v2 site vs the oracle chain, no autograd; the generic path's error beside it; either switch off = today's generic path"""
    worst = {}
    for self_attn in (True, False):
        s = build_site(self_attn, arrangement, dev, **shape)
        p = s["p_main"]
        tag = f"{arrangement}/{'self' if self_attn else 'cross'}"
        yo = check_site_can_see(s, tag)
        with torch.no_grad():
            y_gen = MC.product_site(s)                                  # both switches at their defaults
            for fold_chain, members in ((True, False), (False, True), (False, False)):
                p.fold_chain, p.fold_control_members = fold_chain, members
                assert p._fold_blocker() is not None and p._needs_generic_path()
                assert torch.equal(MC.product_site(s), y_gen) and states(p) == [], (tag, fold_chain, members, states(p))
            y_fused = MC.product_site(s, fused=True)
            assert p._fold_blocker() is None and not p._needs_generic_path(), p._fold_blocker()
            assert states(p) == ["_chain", "_fold"], states(p)
            n_v2 = 1 + sum(isinstance(m, M.ControlLoRACrossAttnProcessorV2) for m in p._chain_members())
            assert all(len(p.__dict__["_chain"][side][0]) == n_v2 for side in ("in", "out"))
        e_fused, e_gen = rel(y_fused, yo), rel(y_gen, yo)
        print(f"MULTI_CONTROL_V2_SITE {tag}: fused {e_fused:.3e}  generic {e_gen:.3e}  (limit {TOL_Y})")
        assert e_fused < TOL_Y, (tag, e_fused)
        worst[tag] = (e_fused, e_gen)
    return worst


BLOCKERS = ("autograd on", "member with a chain", "member rank 17", "no control states", "v1 member", "nine v2 processors")


def check_blocker(what, self_attn, dev):
    """each reports a reason and produces the generic output bit for bit, and no fold or chain state appears"""
    if what == "v1 member":
        s = MC.build_site(self_attn, "control_pre", dev, main="v2")
    elif what == "nine v2 processors":
        s = build_site(self_attn, "many_members", dev, n_members=8)
    else:
        s = build_site(self_attn, "two_members", dev, **(dict(member_rank=17) if what == "member rank 17" else {}))
    p = s["p_main"]
    grad = what == "autograd on"
    if what == "member with a chain":
        p.pre_loras[0].inject_pre_lora(M.LoRACrossAttnProcessor(64, p.cross_attention_dim, rank=4).to(dev))
    off = MC.product_site(s, fused=False, grad=grad).detach()
    p.fold_chain = p.fold_control_members = True
    if what == "no control states":
        p.pre_loras[0].control_states = None
    with torch.set_grad_enabled(grad):
        why = p._fold_blocker()
        assert why is not None and p._needs_generic_path(), what
    print(f"MULTI_CONTROL_V2_BLOCKER {what}: {why}")
    expect = {"autograd on": "autograd", "member with a chain": "chain of its own", "member rank 17": "rank above 16",
              "no control states": "no control states", "v1 member": "not version 1", "nine v2 processors": "version-2 control processors"}
    assert expect[what] in why, (what, why)
    if what == "no control states":
        return                                                        # (the generic path asserts on the missing states, as the reference)
    on = MC.product_site(s, grad=grad).detach()
    assert torch.equal(on, off), what
    assert states(p) == [], (what, states(p))


def fresh(s):
    p = copy.deepcopy(s["p_main"])
    for k in ("_fold", "_mix", "_chain"):
        p.__dict__.pop(k, None)
    return p


def call_site(s, p_main=None, scale=SCALE):
    """the site as it stands: unlike multi_control_cases.product_site no control map is injected anew (the main processor's own map
    is part of the chain job: injecting it again is a new guide)"""
    dev = s["dev"]
    e = None if s["e"] is None else s["e"].to(dev)
    with torch.no_grad():
        return (s["p_main"] if p_main is None else p_main)(s["p_attn"], s["h"].clone().to(dev), e, None, scale)


def check_staleness(self_attn, dev):
    """a stale chain job is never served: new member control states and in-place weight changes move the fused output, which again
    agrees with the oracle"""
    s = build_site(self_attn, "two_members", dev)
    p = s["p_main"]
    p.fold_chain = p.fold_control_members = True

    p.inject_control_states(MC.tokens(s["ctrl"], dev))        # once: the main processor's own map is part of the job

    def out(p_main=None, scale=SCALE):
        return call_site(s, p_main, scale)
    y0 = out()
    ch0, gen0 = p.__dict__["_chain"], p.__dict__["_fold"]["gen"]
    assert torch.equal(y0, out()) and p.__dict__["_chain"] is ch0 and p.__dict__["_fold"]["gen"] == gen0, "an unchanged site rebuilds nothing"
    MC.inject_member_controls(s, scale_by=-0.5)               # a new guide
    y1 = out()
    assert p.__dict__["_chain"] is not ch0 and p.__dict__["_fold"]["gen"] == gen0, "new control states rebuild the job, not the fold"
    yo = MC.oracle_site(s)
    assert rel(y1, yo) < TOL_Y and rel(y0, yo) > 2 * TOL_Y, (rel(y1, yo), rel(y0, yo))
    assert torch.equal(y1, out(fresh(s)))
    ch1 = p.__dict__["_chain"]
    with torch.no_grad():                                     # an in-place change of a member's control up matrix: G is stale
        p.pre_loras[0].to_control.up.weight.mul_(-1.5)
        s["o_main"].pre_loras[0].to_control.up.weight.mul_(-1.5)
    y2 = out()
    yo2 = MC.oracle_site(s)
    assert p.__dict__["_chain"] is not ch1
    assert rel(y2, yo2) < TOL_Y and rel(y1, yo2) > 2 * TOL_Y, (rel(y2, yo2), rel(y1, yo2))
    assert torch.equal(y2, out(fresh(s)))
    p.post_loras.clear()                                      # the chain edited
    s["o_main"].post_loras.clear()
    y3 = out()
    assert not torch.equal(y3, y2) and torch.equal(y3, out(fresh(s))) and rel(y3, MC.oracle_site(s)) < TOL_Y
    y4 = out(scale=0.3)                                       # another scale
    assert not torch.equal(y4, y3) and torch.equal(y4, out(fresh(s), scale=0.3))
    ch4 = p.__dict__["_chain"]
    p.inject_control_states(MC.tokens((s["ctrl"].float() * 0.5).half(), dev))      # a new guide for the main model
    y5 = out(scale=0.3)
    assert p.__dict__["_chain"] is not ch4 and not torch.equal(y5, y4) and torch.equal(y5, out(fresh(s), scale=0.3))
    return s


# ------------------------------------------------------------------------------------------------ reference records
V2_RECORD_CASES = ("v2.member_pre", "v2.member_post")


def replay_record_fused(name, rec, dev="cpu"):
    """multi_control_cases.replay_record's product side with both switches on, under no_grad -> (y, recorded y, main processor)"""
    from controllora_amd import unet as U
    case, where, _ = name.split(":")
    self_attn = where == "self"
    C, heads, ctx = MC.GEOM["C"], MC.GEOM["heads"], MC.GEOM["ctx"]
    cad = None if self_attn else ctx
    mods = dict(control=M.ControlLoRACrossAttnProcessor, control_v2=M.ControlLoRACrossAttnProcessorV2, plain=M.LoRACrossAttnProcessor)
    attn = U.CrossAttention(C, cad, heads=heads, dim_head=C // heads)
    main, members = MC.record_chain(case, self_attn, mods)
    MC._load_prefixed(attn, rec, "attn.")
    MC._load_prefixed(main, rec, "main.")
    for i, m in enumerate(members):
        MC._load_prefixed(m, rec, f"member{i}.")
    h, e = rec["h"], rec.get("e")
    attn.to(dev); main.to(dev)
    main.inject_control_states(MC.tokens(rec["ctrl.main"].half(), dev))
    for i, m in enumerate(members):
        m.to(dev)
        m.requires_grad_(False)
        if f"ctrl.member{i}" in rec:
            m.inject_control_states(MC.tokens(rec[f"ctrl.member{i}"].half(), dev))
    main.fold_chain = main.fold_control_members = True
    with torch.no_grad():
        assert main._fold_blocker() is None, main._fold_blocker()
        y = main(attn, h.half().to(dev), None if e is None else e.half().to(dev), None, MC.GEOM["scale"])
    assert states(main) == ["_chain", "_fold"]
    return y, rec["y"], main


# ------------------------------------------------------------------------------------------------ whole small UNets
def check_two_control_unet(dev):
    """one forward of the small topology under two v2 control models: fused and generic against the oracle chain; the fused forward
    makes exactly two chain launches per attention site and fewer library calls than the generic one"""
    inp = MC.small_inputs()
    g = torch.Generator().manual_seed(9)
    guides = [inp["guide"], torch.rand(inp["guide"].shape, generator=g) * 2 - 1]
    o_unet, o_cl, p_unet, p_cl = MC.two_control_small_pair(dev, fold=True, case="v2")
    with torch.no_grad():
        for oc, gd in zip(o_cl, guides):
            oc(gd[:1])
        yo = o_unet(inp["latents"], 501, inp["ehs"]).sample
    MC.forward(p_unet, p_cl, inp, guides, dev)                 # warm: lazy packs, the fold, the jobs
    with torch.no_grad():
        rep = p_cl[0].fold_report()
    assert all(r["folded"] and r["control_members"] == 1 for r in rep.values()), rep
    with count_library_calls() as names:
        y_fused = MC.forward(p_unet, p_cl, inp, guides, dev)
    sites = len(p_unet.attn_processors)
    assert names.count("clora_control_chain_f16") == 2 * sites, (names.count("clora_control_chain_f16"), sites)
    assert "clora_lora_fold_f16" not in names
    y_other = MC.forward(p_unet, p_cl, inp, [guides[0], -guides[1]], dev)
    p_cl[0].fold_chains(False)
    assert all(states(p) == [] for _, p in p_cl[0]._named_processors())
    MC.forward(p_unet, p_cl, inp, guides, dev)
    with count_library_calls() as generic_names:
        y_gen = MC.forward(p_unet, p_cl, inp, guides, dev)
    e_fused, e_gen = rel(y_fused, yo), rel(y_gen, yo)
    print(f"LAUNCHES small topology, two v2 controls: fused {len(names)} library calls per forward (control_chain "
          f"{names.count('clora_control_chain_f16')}), generic {len(generic_names)}, sites {sites}")
    print(f"TWO_CONTROL_V2 small UNet forward vs oracle chain: fused {e_fused:.3e}  generic {e_gen:.3e}  (limit {UNET_LIMIT});  "
          f"another member guide moves the output by {rel(y_other, y_fused):.3e}")
    assert "clora_control_chain_f16" not in generic_names and len(names) < len(generic_names), (len(names), len(generic_names))
    assert rel(y_other, y_fused) > 10 * e_fused, "the second control model must matter"
    assert e_fused < UNET_LIMIT and e_gen < UNET_LIMIT, (e_fused, e_gen)


_SAMPLER_ORACLE = {}


def two_control_sampler_case(dev, res=128, steps=50, guidance_scale=9.0, nb=2, ctx_dim=64, ctx_len=7, seed=5):
    """multi_control_cases.two_control_sampler_case for two v2 control models: computed once per process"""
    from tests import full_cases as F
    if "case" in _SAMPLER_ORACLE:
        return _SAMPLER_ORACLE["case"]
    g = torch.Generator().manual_seed(seed)
    L = res // 8
    guides = [((torch.rand(1, 3, res, res, generator=g) > 0.9).float() * 2 - 1) for _ in range(2)]
    cond = torch.randn(nb, ctx_len, ctx_dim, generator=g).half().float()
    uncond = torch.randn(nb, ctx_len, ctx_dim, generator=g).half().float()
    lat0 = torch.randn(nb, 4, L, L, generator=g).half().float()
    o_unet, o_cl, _, _ = pair = MC.two_control_small_pair(dev, fold=True, case="v2")
    with torch.no_grad():
        ref, _ = F.oracle_ddim(o_unet, MC._OracleControls(o_cl, guides), None, cond, uncond, steps, guidance_scale, lat0)

        def low_precision(where):
            h_unet, h_cl = copy.deepcopy((o_unet, o_cl))
            h_unet.half().to(where)
            for m in h_cl:
                m.half().to(where)
            mv = lambda t: t.half().to(where)
            out, _ = F.oracle_ddim(h_unet, MC._OracleControls(h_cl, guides), None, mv(cond), mv(uncond), steps, guidance_scale, mv(lat0))
            return out.float().cpu()

        try:
            low = low_precision(dev)
        except RuntimeError as e:                           # an oracle module that builds a tensor on the host: the host loop instead
            print("NOTE two_control_sampler_case (v2): the fp16 oracle failed on", dev, "->", str(e).splitlines()[0][:200])
            low = low_precision("cpu")
    case = dict(guides=guides, cond=cond, uncond=uncond, lat0=lat0, ref=ref, floor=rel(low, ref), steps=steps,
                guidance_scale=guidance_scale, pair=pair)
    _SAMPLER_ORACLE["case"] = case
    return case
