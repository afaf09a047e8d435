"""Record what clora_gemm_f16_ex does for every tile_cfg value 0..99 on the host emulator build (tests/hipemu): return code (or
the exception class kernels.gemm raises) and the SHA-1 of every output tensor, for each kind of launch whose dispatch depends on
the tile -- plain, fused epilogue, split-K, GEGLU forward / backward, the in-launch adapter down-projection at four segment widths,
the fused LayerNorm, a 3x3 conv the patch kernel can take and one it cannot, and the raw calls whose return codes kernels.gemm
hides.  tests/test_gemm_dispatch_emu.py replays the sweep against tests/golden/gemm_dispatch_emu.json: a change of the host
dispatch that moves any launch to another kernel, or changes what is refused, shows there.  Uses only calls that are older than
the tile table, so the same file records the fixture from an older tree:
    python tools/gemm_dispatch_record.py [--out tests/golden/gemm_dispatch_emu.json]"""
import argparse
import ctypes as C
import hashlib
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import torch  # noqa: E402

f16, f32 = torch.float16, torch.float32
FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_dispatch_emu.json")


def _sha(t):
    return None if t is None else hashlib.sha1(t.contiguous().numpy().tobytes()).hexdigest()


def _rnd(shape, g, scale=1.0, dtype=f16):
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def sweep(cfgs=range(100)):
    """-> {"<kind>/<tile_cfg>": [return code or exception class, sha1 of every output]}; the emulator must be the active library"""
    from controllora_amd import capi, kernels as K, ops
    g = torch.Generator().manual_seed(1234)
    M, N, Kd = 150, 144, 128
    A, B = _rnd((M, Kd), g), _rnd((N, Kd), g, 1 / math.sqrt(Kd))
    bias, res = _rnd((N,), g, dtype=f32), _rnd((M, N), g)
    T4, U4 = _rnd((M, 4), g, dtype=f32), _rnd((N, 4), g, dtype=f32)
    A3, B3 = _rnd((M, 224), g), _rnd((N, 224), g, 1 / math.sqrt(224))       # 7 BK-32 steps, 4 BK-64 steps: the slabs differ
    # GEGLU: F = 64 (forward N = 2F, backward N = F)
    Bg, bg = _rnd((128, Kd), g, 1 / math.sqrt(Kd)), _rnd((128,), g, dtype=f32)
    Bd, hg = _rnd((64, Kd), g, 1 / math.sqrt(Kd)), _rnd((M, 128), g)
    # in-launch down-projection: one segment of 128 / 192 / 320 columns, two of 64
    fused = {}
    for seg, nseg in ((64, 2), (128, 1), (192, 1), (320, 1)):
        Ds = [_rnd((4, Kd), g, 1 / math.sqrt(Kd), dtype=f32) for _ in range(nseg)]
        fused[seg] = (_rnd((seg * nseg, Kd), g, 1 / math.sqrt(Kd)), _rnd((seg * nseg, 4), g, dtype=f32), ops.ADAPTER_PACKS.get(Ds), nseg)
    # LayerNorm at N = 320
    Al, Bl = _rnd((M, 64), g), _rnd((320, 64), g, 0.1)
    gamma, beta = 1 + 0.2 * _rnd((320,), g, dtype=f32), 0.2 * _rnd((320,), g, dtype=f32)
    # 3x3 convs: 2 x 8 x 8, 64 -> 64 channels, stride 1 (patch-eligible at 128 pixels); 1 x 8 x 8, 16 -> 24, stride 2 (never)
    xp, wp = _rnd((128, 64), g), ops.conv_k_order(_rnd((64, 9, 64), g, 1 / 24.0), 64)
    cdp, _, _ = K.conv_fwd_desc(8, 8, 64, 3, 1, 1, kchunk=64)
    xs, ws = _rnd((64, 16), g), _rnd((24, 9 * 16), g, 1 / 12.0)
    cds, _, _ = K.conv_fwd_desc(8, 8, 16, 3, 2, 1)
    cdll, p = capi.lib().cdll, capi.ptr

    def via_gemm(fn):
        try:
            outs = fn()
        except Exception as e:                                    # noqa: BLE001  (the class is what is recorded)
            return [type(e).__name__]
        return [0] + [_sha(t) for t in (outs if isinstance(outs, tuple) else (outs,))]

    def raw(Aop, lda, Bop, out, M_, N_, K_, epi, cfg, extra=()):
        rc = cdll.clora_gemm_f16_ex(p(Aop), lda, p(Bop), p(out) if out is not None else None, N_, M_, N_, K_, None, C.byref(epi), 1, cfg, None, 0, None)
        return [rc] + [_sha(t) for t in ((out,) if out is not None else ()) + tuple(extra)]

    rec = {}
    for cfg in cfgs:
        kw = dict(tile_cfg=cfg, _tuned=False)
        z = lambda *shape: torch.zeros(shape, dtype=f16)          # noqa: E731
        rec[f"plain/{cfg}"] = via_gemm(lambda: K.gemm(A, B, M, N, Kd, out=z(M, N), split_k=1, **kw))
        rec[f"epilogue/{cfg}"] = via_gemm(lambda: K.gemm(A, B, M, N, Kd, out=z(M, N), split_k=1, bias=bias, residual=res, lora_t=T4, lora_u=U4,
                                                          lora_seg=N, lora_scale=0.7, **kw))
        rec[f"split3/{cfg}"] = via_gemm(lambda: K.gemm(A3, B3, M, N, 224, out=z(M, N), split_k=3, **kw))
        rec[f"geglu_fwd/{cfg}"] = via_gemm(lambda: K.gemm(A, Bg, M, 128, Kd, bias=bg, geglu=1, geglu_y=z(M, 64), **kw))
        rec[f"geglu_bwd/{cfg}"] = via_gemm(lambda: K.gemm(A, Bd, M, 64, Kd, geglu=2, geglu_h=hg, out=z(M, 128), **kw))
        for seg, (Bf, Uf, pack, nseg) in fused.items():
            def run():
                T = torch.zeros((M, 4 * nseg), dtype=f32)
                return K.gemm(A, Bf, M, seg * nseg, Kd, out=z(M, seg * nseg), split_k=1, lora_t=T, lora_u=Uf, lora_seg=seg, lora_scale=0.7,
                              lora_r=4, lora_dpack=pack, **kw), T
            rec[f"fused_down{seg}/{cfg}"] = via_gemm(run)

        def run_ln():
            slot = K.LayerNormSlot(gamma, beta, 1e-5)
            return K.gemm(Al, Bl, M, 320, 64, out=z(M, 320), split_k=1, ln=slot, **kw), slot.out
        rec[f"ln/{cfg}"] = via_gemm(run_ln)
        rec[f"conv_patch/{cfg}"] = via_gemm(lambda: K.gemm(xp, wp, 128, 64, 576, conv=cdp, out=z(128, 64), split_k=1, **kw))
        rec[f"conv_stride2/{cfg}"] = via_gemm(lambda: K.gemm(xs, ws, 16, 24, 144, conv=cds, out=z(16, 24), split_k=1, **kw))
        # raw: what kernels.gemm decides before the library sees the launch
        e = capi.Epilogue()
        y = z(M, 64)
        e.geglu, e.geglu_f, e.geglu_y = 1, 64, p(y)
        rec[f"raw_geglu_fwd/{cfg}"] = raw(A, Kd, Bg, z(M, 128), M, 128, Kd, e, cfg, (y,))
        e, lo = capi.Epilogue(), z(M, 320)
        e.ln_gamma, e.ln_beta, e.ln_out, e.ln_eps = p(gamma), p(beta), p(lo), 1e-5
        rec[f"raw_ln/{cfg}"] = raw(Al, 64, Bl, z(M, 320), M, 320, 64, e, cfg, (lo,))
        rec[f"raw_plain/{cfg}"] = raw(A, Kd, B, z(M, N), M, N, Kd, capi.Epilogue(), cfg)
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    from tests.emu_fixture import use_emulator
    with use_emulator():
        rec = sweep()
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
    print("wrote", args.out, len(rec), "cases")
