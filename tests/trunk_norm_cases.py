"""Norms that read the compensated trunk (CLORA_TRUNK_LO=norms; include/clora.h clora_groupnorm_fwd_f16_lo / clora_layernorm_fwd_f16_lo),
shared by the host-emulator and the GPU test modules.

Inputs of the kernel cases: v drawn in fp32 with unit variance around `offset`, hi = fp16(v), lo = fp16(v - hi) -- what a launch that
writes a residual sum leaves behind (clora_epilogue_t.c_lo).  The reference is the fp64 norm of double(hi) + double(lo).  Limits:
  - with lo, output and statistics within 8e-4 of the reference: the limits the same kernels carry against fp64 without a remainder
    (kernel_cases.case_groupnorm_offset); the fp16 rounding of the output alone is 2.1e-4;
  - the plain call (hi only) on the same data at offset 10 is ABOVE 1.5e-3: fp16 has a spacing of 2^-7 at 10, so hi is a uniform error of
    2^-7 / sqrt(12) = 2.26e-3 std away from v, added to the output's own rounding: 2.2e-3 -- a kernel that ignores lo lands there;
  - at offset 0 the error with lo is strictly below the plain call's, measured on the same data (2.1e-4 against 2.9e-4).
Every case prints the figures it asserts on."""
import math

import pytest
import torch
import torch.nn.functional as F

from controllora_amd import capi
from controllora_amd import kernels as K
from tests import kernel_cases as KC

f16, f32 = torch.float16, torch.float32
rel64, no_outliers, options = KC.rel64, KC.no_outliers, KC.options

Y_LIMIT = STAT_LIMIT = 8e-4
PLAIN_FLOOR = 1.5e-3


def split_hi_lo(v):
    hi = v.half()
    return hi, (v - hi.float()).half()


def _affine(C, dev, g):
    return (1 + 0.2 * KC.rnd((C,), dev, g, dtype=f32)), 0.2 * KC.rnd((C,), dev, g, dtype=f32)


def _gn64(x64, G, gamma, beta, eps, silu):
    y = F.group_norm(x64.permute(0, 2, 1), G, gamma.double().cpu(), beta.double().cpu(), eps).permute(0, 2, 1)
    return F.silu(y) if silu else y


def case_groupnorm_lo(dev, B, HW, C, G, silu=False, eps=1e-5, seed=71):
    """every plan the shape can take ("gn_resident" 0 / 1 x "gn_team" 0 / 2), offsets 10 and 0.  With SiLU the plain-call floor is not
    asserted (the activation flattens the negative half of the output, the figure of the module docstring is for the bare norm)."""
    g = torch.Generator().manual_seed(seed)
    gamma, beta = _affine(C, dev, g)
    for offset in (10, 0):
        hi, lo = split_hi_lo(KC.rnd((B, HW, C), dev, g, dtype=f32) + offset)
        x64 = hi.double().cpu() + lo.double().cpu()
        y = _gn64(x64, G, gamma, beta, eps, silu)
        xg = x64.reshape(B, HW, G, C // G)
        mean, rstd = xg.mean((1, 3)), (xg.var((1, 3), unbiased=False) + eps).rsqrt()
        zero = torch.zeros_like(lo)
        for resident in (0, 1):
            for team in (0, 2):
                with options(gn_resident=resident, gn_team=team):
                    out, stats = K.groupnorm_fwd(hi, gamma, beta, G, eps, silu, x_lo=lo)
                    out2, stats2 = K.groupnorm_fwd(hi, gamma, beta, G, eps, silu, x_lo=lo)
                    plain, pstats = K.groupnorm_fwd(hi, gamma, beta, G, eps, silu)
                    none, nstats = K.groupnorm_fwd(hi, gamma, beta, G, eps, silu, x_lo=None)
                    zer, zstats = K.groupnorm_fwd(hi, gamma, beta, G, eps, silu, x_lo=zero)
                errs = dict(y=rel64(out, y), mean=rel64(stats[..., 0], mean), rstd=rel64(stats[..., 1], rstd), plain=rel64(plain, y))
                print(f"GN_LO {(B, HW, C, G)} offset={offset} silu={silu} gn_resident={resident} gn_team={team} " +
                      " ".join(f"{k_}={v_:.2e}" for k_, v_ in errs.items()))
                assert all(math.isfinite(v_) for v_ in errs.values()), errs
                if offset:
                    assert errs["y"] < Y_LIMIT and errs["mean"] < STAT_LIMIT and errs["rstd"] < STAT_LIMIT, (resident, team, errs)
                    no_outliers(out, y, "groupnorm of hi + lo")
                    if not silu:
                        assert errs["plain"] > PLAIN_FLOOR, (resident, team, errs)           # the control: hi alone is not enough
                else:
                    assert errs["y"] < errs["plain"], (resident, team, errs)
                assert torch.equal(out, out2) and torch.equal(stats, stats2)                 # two launches, the same bits
                assert torch.equal(none, plain) and torch.equal(nstats, pstats)              # no remainder: the call of before
                assert torch.equal(zer, plain) and torch.equal(zstats, pstats)               # an all-zero remainder changes no bit
    assert K.gn_team_errors(hi.device) == 0


def case_groupnorm_lo_concat(dev, B, HW, Ca, Cb, G, silu, eps=1e-5, seed=72):
    """the concatenating form with both remainders, only x_lo, only x2_lo (Ca != Cb in the shape lists: a remainder read at the other
    half's pitch would show): against fp64 of what was given, and bit for bit against the materialised concatenation with the
    concatenated remainder (zeros where a half has none); xcat stays the concatenation of the hi halves."""
    g = torch.Generator().manual_seed(seed)
    a, a_lo = split_hi_lo(KC.rnd((B, HW, Ca), dev, g, dtype=f32) * 1.5 + 10)
    b, b_lo = split_hi_lo(KC.rnd((B, HW, Cb), dev, g, dtype=f32) * 0.7 - 10)
    gamma, beta = _affine(Ca + Cb, dev, g)
    xc = torch.cat([a, b], -1).contiguous()
    for use_a, use_b in ((True, True), (True, False), (False, True)):
        la, lb = (a_lo if use_a else None), (b_lo if use_b else None)
        lc = torch.cat([a_lo if use_a else torch.zeros_like(a), b_lo if use_b else torch.zeros_like(b)], -1).contiguous()
        y = _gn64(xc.double().cpu() + lc.double().cpu(), G, gamma, beta, eps, silu)
        for resident in (0, 1):
            for team in (0, 2):
                with options(gn_resident=resident, gn_team=team):
                    out, stats, xcat = K.groupnorm_fwd(a, gamma, beta, G, eps, silu, x2=b, x_lo=la, x2_lo=lb)
                    out_m, stats_m = K.groupnorm_fwd(xc, gamma, beta, G, eps, silu, x_lo=lc)
                    plain, _, _ = K.groupnorm_fwd(a, gamma, beta, G, eps, silu, x2=b)
                e, ep = rel64(out, y), rel64(plain, y)
                print(f"GN_LO_CAT {(B, HW, Ca, Cb, G)} x_lo={use_a} x2_lo={use_b} gn_resident={resident} gn_team={team} y={e:.2e} plain={ep:.2e}")
                assert e < Y_LIMIT, (use_a, use_b, resident, team, e)
                no_outliers(out, y, "concatenating groupnorm of hi + lo")
                assert torch.equal(xcat, xc)
                assert torch.equal(out, out_m) and torch.equal(stats, stats_m)
                if not silu and use_a and use_b:                  # (the floor is derived for an input that lacks its remainder everywhere)
                    assert ep > PLAIN_FLOOR, (use_a, use_b, ep)


def case_groupnorm_lo_rejects_deferred(dev, B=2, HW=64, C=128, Kd=256, G=8, split=4, seed=73):
    """a deferred split-K source and a remainder never meet (a launch that writes c_lo is never deferred): CLORA_ERR_ARG, nothing is
    launched.  First at the entry point with a hand-made descriptor (runs whatever CLORA_DEFER_FINISH says), then through the wrapper with
    a real deferred GEMM (only when finishes are deferred at all)."""
    import ctypes
    g = torch.Generator().manual_seed(seed)
    M = B * HW
    A, Wt = KC.rnd((M, Kd), dev, g), (KC.rnd((C, Kd), dev, g).float() * 0.1).half()
    gamma, beta = _affine(C, dev, g)
    lo = torch.zeros((B, HW, C), dtype=f16, device=dev)
    assert not K._PENDING
    ref = K.gemm(A, Wt, M, C, Kd, split_k=split)

    def entry(src, x_lo):
        y = torch.empty((B, HW, C), dtype=f16, device=dev)
        stats = torch.empty((B, G, 2), dtype=f32, device=dev)
        ws, team = K._gn_ws(B, HW, C, G, lo.device, False, False), K.gn_team_state(lo.device)
        rc = capi.lib().cdll.clora_groupnorm_fwd_f16_lo(
            capi.ptr(ref, f16), None, 0, ctypes.byref(src), None, capi.ptr(y), capi.ptr(gamma, f32), capi.ptr(beta, f32), capi.ptr(stats), B, HW, C,
            G, 1e-5, 1, capi.ptr(team), team.numel(), capi.ptr(ws), ws.numel(), capi.ptr(x_lo, f16) if x_lo is not None else None, None,
            capi.stream())
        return rc, y

    slabs = torch.zeros((2, M, C), dtype=f32, device=dev)
    d = capi.Deferred()
    d.partial, d.splits, d.M, d.N, d.C, d.ldc = capi.ptr(slabs), 2, M, C, capi.ptr(ref), C
    assert entry(d, lo)[0] == capi.ERR_ARG
    d.splits = 0                                                  # not deferred after all: the same call is taken
    rc, y_entry = entry(d, lo)
    assert rc == capi.OK
    y0, _ = K.groupnorm_fwd(ref.reshape(B, HW, C), gamma, beta, G, 1e-5, True)
    assert torch.equal(y_entry, y0)

    out = K.gemm(A, Wt, M, C, Kd, split_k=split, defer=True)
    assert bool(K._PENDING) == K.DEFER_FINISH
    if K._PENDING:                                                # (CLORA_DEFER_FINISH=0: nothing is ever pending, the check above stands alone)
        with pytest.raises(capi.CloraError):
            K.groupnorm_fwd(out.reshape(B, HW, C), gamma, beta, G, 1e-5, True, x_lo=lo)
        # the wrapper took the entry out of _PENDING before the library refused it: `out` is never finished and is not read again
        assert not K._PENDING
    # the same tensor finished: the remainder is taken
    out = K.gemm(A, Wt, M, C, Kd, split_k=split)
    y1, _ = K.groupnorm_fwd(out.reshape(B, HW, C), gamma, beta, G, 1e-5, True, x_lo=lo)
    assert torch.equal(y0, y1)


def case_layernorm_lo(dev, M, C, seed=74):
    """both LayerNorm forward kernels ("ln_rows" 1: several rows per wave, 0: one row per wave), offsets 10 and 0"""
    g = torch.Generator().manual_seed(seed)
    gamma, beta = _affine(C, dev, g)
    for offset in (10, 0):
        hi, lo = split_hi_lo(KC.rnd((M, C), dev, g, dtype=f32) + offset)
        y = F.layer_norm(hi.double().cpu() + lo.double().cpu(), (C,), gamma.double().cpu(), beta.double().cpu(), 1e-5)
        zero = torch.zeros_like(lo)
        try:
            for rows in (0, 1):
                K.set_option("ln_rows", rows)
                out, out2 = K.layernorm_fwd(hi, gamma, beta, 1e-5, x_lo=lo), K.layernorm_fwd(hi, gamma, beta, 1e-5, x_lo=lo)
                plain = K.layernorm_fwd(hi, gamma, beta, 1e-5)
                none, zer = K.layernorm_fwd(hi, gamma, beta, 1e-5, x_lo=None), K.layernorm_fwd(hi, gamma, beta, 1e-5, x_lo=zero)
                e, ep = rel64(out, y), rel64(plain, y)
                print(f"LN_LO {(M, C)} offset={offset} ln_rows={rows} y={e:.2e} plain={ep:.2e}")
                if offset:
                    assert e < Y_LIMIT, (rows, e)
                    no_outliers(out, y, "layernorm of hi + lo")
                    assert ep > PLAIN_FLOOR, (rows, ep)
                else:
                    assert e < ep, (rows, e, ep)
                assert torch.equal(out, out2) and torch.equal(none, plain) and torch.equal(zer, plain)
        finally:
            K.set_option("ln_rows", 1)                            # the library default


# ---------------------------------------------------------------------------------------------------------------- blocks
class call_counter:
    """counts calls per entry point at the binding (capi.Lib.call) for the block"""

    def __init__(self):
        self.n = {}

    def __enter__(self):
        self.orig = capi.Lib.call
        counter, orig = self.n, self.orig

        def call(lib, name, *args):
            counter[name] = counter.get(name, 0) + 1
            return orig(lib, name, *args)
        capi.Lib.call = call
        return self

    def __exit__(self, *exc):
        capi.Lib.call = self.orig
        return False

    def lo_calls(self):
        return self.n.get("clora_groupnorm_fwd_f16_lo", 0) + self.n.get("clora_layernorm_fwd_f16_lo", 0)


def _seeded_(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.ndim >= 2:
                p.copy_(torch.randn(p.shape, generator=g) / math.sqrt(p[0].numel()))
            elif name.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))


def _offset_trunk(B, N, C, dev, g):
    """a trunk tensor with per-channel offsets of 10 std and its remainder"""
    v = torch.randn((B, N, C), generator=g) + 10.0 * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    hi, lo = split_hi_lo(v)
    return hi.to(dev).contiguous(), lo.to(dev).contiguous()


def case_blocks_norms(dev, seed=75):
    """one Transformer2DModel and one ResnetBlock2D of the small topology inside TrunkLo(True, norms=True), their input's remainder
    registered by hand: closer to the fp32 torch block evaluated on hi + lo than the same block under TrunkLo(True)."""
    from controllora_amd import unet as U
    from oracle import unet_ref
    g = torch.Generator().manual_seed(seed)
    B, H, W, C, ctx = 2, 8, 8, 64, 64
    errs = {}
    for kind in ("transformer", "resnet"):
        if kind == "transformer":
            ref = unet_ref.Transformer2DModel(4, C // 4, C, ctx, 8)
            blk = U.Transformer2DModel(4, C // 4, C, ctx, 8)
        else:
            ref = unet_ref.ResnetBlock2D(C, 128, 128, 8, 1e-5)
            blk = U.ResnetBlock2D(C, 128, 128, 8, 1e-5)
        _seeded_(ref, seed + 1)
        blk.load_state_dict({k: v for k, v in ref.state_dict().items()})
        blk.to(dev)
        ref_h = ref.half().float()                                # the fp16-rounded weights the product block carries, evaluated in fp32
        hi, lo = _offset_trunk(B, H * W, C, dev, g)
        x32 = (hi.float().cpu() + lo.float().cpu()).reshape(B, H, W, C).permute(0, 3, 1, 2)
        ehs = torch.randn((B, 7, ctx), generator=g).half()
        temb = torch.randn((B, 128), generator=g).half()
        with torch.no_grad():
            if kind == "transformer":
                want = ref_h(x32, ehs.float())
            else:
                want = ref_h(x32, temb.float())
            want = want.permute(0, 2, 3, 1).reshape(B, H * W, -1)
            got = {}
            for mode in ("infer", "norms"):
                with K.TrunkLo(True, norms=mode == "norms"), call_counter() as cc:
                    K._TRUNK_LO[hi.data_ptr()] = (hi.reshape(B * H * W, C), lo.reshape(B * H * W, C))
                    if kind == "transformer":
                        out = blk(hi, ehs.to(dev), {})
                    else:
                        out = blk(hi, F.silu(temb.float()).half().to(dev), H, W)
                    rem = K._TRUNK_LO.get(out.data_ptr())
                    full = out.float().cpu() + (rem[1].float().cpu().reshape(out.shape) if rem is not None else 0)
                assert not K._TRUNK_LO and not K._TRUNK_LO_ON[0] and not K._TRUNK_NORMS[0]
                assert (cc.lo_calls() > 0) == (mode == "norms"), (kind, mode, cc.n)
                got[mode] = KC.rel(full, want)
        print(f"BLOCK_NORMS {kind}: infer={got['infer']:.3e} norms={got['norms']:.3e}")
        assert got["norms"] < got["infer"], (kind, got)
        errs[kind] = got
    return errs


def case_small_unet_modes(dev, monkeypatch, case="v1"):
    """cases.SMALL_UNET with the inputs of e2e_cases.check_inference_broadcast: mode "infer" never reaches a `_lo` entry point and equals a
    forward under TrunkLo(True) bit for bit; mode "norms" reaches them and is closer to the fp32 oracle."""
    from oracle import cases
    from tests import e2e_cases as E
    inp = cases.seeded_inputs()
    o_unet, _, o_clora = cases.build_oracle_case(case)
    unet, _, clora = E.build_product_case(case, dev)
    guide = inp["guide"][:1]
    lat = torch.cat([inp["latents"][:1]] * 2)
    ehs = inp["ehs"][:2]
    res = {}
    with torch.no_grad():
        o_clora(guide)
        clora(guide.to(dev).to(f16))
        refs = [o_unet(lat, t, ehs).sample for t in (801, 401)]
        for mode in ("infer", "norms"):
            monkeypatch.setattr(K, "TRUNK_LO_MODE", mode)
            with call_counter() as cc:
                outs = [unet(lat.to(dev).to(f16), t, ehs.to(dev).to(f16)).sample for t in (801, 401)]
            res[mode] = (outs, cc.lo_calls(), sum(cc.n.values()), max(E.rel(o, r) for o, r in zip(outs, refs)))
            assert not K._TRUNK_LO and not K._TRUNK_NORMS[0]
    print(f"SMALL_UNET_NORMS {case}: infer err={res['infer'][3]:.4e} ({res['infer'][2]} library calls for 2 forwards, {res['infer'][1]} `_lo`), "
          f"norms err={res['norms'][3]:.4e} ({res['norms'][2]} library calls, {res['norms'][1]} `_lo`)")
    assert res["infer"][1] == 0 and res["norms"][1] > 0
    assert res["norms"][3] < res["infer"][3], (res["infer"][3], res["norms"][3])
    return unet, clora, inp, res


def check_infer_is_trunklo_true(unet, inp, dev, monkeypatch):
    """mode "infer" == the TrunkLo(True) window of before: the same forward with the UNet's own window switched off and the window opened by
    hand gives the same bits"""
    lat = torch.cat([inp["latents"][:1]] * 2).to(dev).to(f16)
    ehs = inp["ehs"][:2].to(dev).to(f16)
    with torch.no_grad():
        monkeypatch.setattr(K, "TRUNK_LO_MODE", "infer")
        a = unet(lat, 801, ehs).sample
        monkeypatch.setattr(K, "TRUNK_LO_MODE", "off")
        with K.TrunkLo(True):
            b = unet(lat, 801, ehs).sample
        c = unet(lat, 801, ehs).sample
    assert torch.equal(a, b)
    assert not torch.equal(a, c)                                  # (and the window does something)
