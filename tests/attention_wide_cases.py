"""Forward attention at head dims 160 < D <= 512 (clora_attn_wide.hip behind clora_attn_fwd_f16): the cases shared by the host-emulator
and the GPU test modules.  Every case compares K.attn_fwd with fp64 on the same fp16 inputs under the limits the narrow kernels are held
to (tests/kernel_cases.py::attention_full_check): o within 2e-3 norm-wise and elementwise without outliers, the LSE under the per-row
bound of the one fp16 rounding of the scaled query, and every element of o written (the buffers start as NaN)."""
import os

import pytest
import torch

from controllora_amd import capi, kernels as K
from tests import kernel_cases as KC

f16, f32 = torch.float16, torch.float32
NAN = float("nan")

# (B, H, Nq, Nk, D): the first six run on the host emulator as well
SHAPES = {
    "whole_tiles": (1, 1, 64, 64, 512),
    "ragged_batch": (2, 1, 200, 200, 512),
    "two_heads": (1, 2, 130, 77, 256),
    "fused_168": (1, 1, 70, 150, 168),
    "ragged_d": (1, 1, 96, 96, 504),
    "one_key": (1, 1, 33, 1, 512),
}
RAMP = (2, 1, 100, 300, 512)
NEGATIVE = (1, 1, 40, 200, 512)
NARROW = (1, 2, 70, 150, 40)
NARROW_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_narrow_fwd_emu.pt")


def check_forward(q, k, v, dims, o=None, tag=""):
    """one launch on prepared inputs (2-D row-strided views) against fp64; `o`: the output view to write (NaN-filled by the caller)"""
    B, H, Nq, Nk, D = dims
    scale = D ** -0.5
    if o is None:
        o = torch.full((B * Nq, H * D), NAN, dtype=f16, device=q.device)
    got, lse = K.attn_fwd(q, k, v, B, H, Nq, Nk, D, scale, out=o)
    assert got is o
    ref = KC._attn_ref64(q, k, v, None, B, H, Nq, Nk, D, scale)
    assert bool(torch.isfinite(o.float()).all()), "not every element of o was written (or a NaN / inf was computed)"
    assert bool(torch.isfinite(lse).all())
    err = KC.rel64(o, ref["o"])
    bound = 2.0 ** -11 * ref["mag"] + 1e-5
    lse_err = (lse.double() - ref["lse"]).abs()
    print(f"ATTN_WIDE{tag} {dims} o={err:.2e} lse={float(lse_err.max()):.2e} lse_margin={float((lse_err / bound).max()):.2f}")
    assert err < 2e-3, ("o", err)
    KC.no_outliers(o, ref["o"], "o")
    assert bool((lse_err <= bound).all()), ("lse", float(lse_err.max()), float(bound.max()))
    return o, lse


def plain_inputs(dev, dims, seed=71):
    B, H, Nq, Nk, D = dims
    g = torch.Generator().manual_seed(seed)
    return KC.rnd((B * Nq, H * D), dev, g), KC.rnd((B * Nk, H * D), dev, g), KC.rnd((B * Nk, H * D), dev, g)


def case_plain(dev, dims):
    return check_forward(*plain_inputs(dev, dims), dims)


def case_fused_168(dev):
    """the first head dim above the old limit (contraction padded from 168 to 512): q, k, v are column blocks of one buffer, o is a
    column block of a wider NaN-filled buffer whose spare columns keep their bits"""
    dims = B, H, Nq, Nk, D = SHAPES["fused_168"]
    g = torch.Generator().manual_seed(72)
    qkv = KC.rnd((Nk, 3 * D + 8), dev, g)
    q, k, v = qkv[:Nq, :D], qkv[:, D:2 * D], qkv[:, 2 * D:3 * D]
    obuf = torch.full((Nq, D + 16), NAN, dtype=f16, device=dev)
    check_forward(q, k, v, dims, o=obuf[:, 8:8 + D], tag=" fused")
    spare = torch.ones(obuf.shape, dtype=torch.bool, device=dev)
    spare[:, 8:8 + D] = False
    assert bool(torch.isnan(obuf[spare].float()).all()), "the forward wrote outside its column block"


STRIDES = (2, 1, 70, 100, 256)


def case_strides(dev, dims=STRIDES):
    """kernel_cases.case_attention_strides for the wide kernel, forward only: q, k, v and o are column blocks (from column 8) of four
    NaN-filled buffers under four different row strides, two batch elements; a K or V tile fetched with the other operand's stride
    brings NaN into o, a store with a wrong stride lands outside o's block"""
    assert dims[4] > K.attn_max_head_dim(True)
    KC.attention_strides_check(KC.attention_strides_inputs(dev, *dims, backward=False), tag=" wide")


def case_one_key(dev):
    """one key: every weight is exactly 1, so every output row is v[0] bit for bit"""
    dims = B, H, Nq, Nk, D = SHAPES["one_key"]
    q, k, v = plain_inputs(dev, dims, seed=73)
    o, lse = check_forward(q, k, v, dims)
    assert torch.equal(o, v[0:1].expand(Nq, D))


def case_ramp(dev, ramp=4.0):
    """as kernel_cases.case_attention(ramp=...): keys grow along the sequence and q is 3x larger, so the rebase path runs on later
    tiles for some queries of a wave and not for others"""
    dims = B, H, Nq, Nk, D = RAMP
    q, k, v = plain_inputs(dev, dims, seed=74)
    w = 1.0 + ramp * torch.arange(Nk, dtype=f32).repeat(B)[:, None] / Nk
    k = (k.float().cpu() * w).to(f16).to(dev)
    q = (q.float() * 3.0).to(f16)
    check_forward(q, k, v, dims, tag=" ramp")


def case_negative_first_tile(dev):
    """as kernel_cases.case_attention_negative_logits: every logit of the first key tile is far below -88 (q = +8, k = -8 on every
    channel), so the still-empty accumulators must not be rescaled by exp2(+huge) = inf; check_forward asserts everything finite"""
    dims = B, H, Nq, Nk, D = NEGATIVE
    g = torch.Generator().manual_seed(75)
    q = torch.full((B * Nq, H * D), 8.0, dtype=f16, device=dev)
    k = KC.rnd((B * Nk, H * D), dev, g, scale=0.05)
    v = KC.rnd((B * Nk, H * D), dev, g)
    k[:64] = -8.0                                            # as there: two of the wide kernel's 32-key tiles
    check_forward(q, k, v, dims, tag=" negative")


def case_repeat_and_block_order(dev, dims):
    """repeat launches and the XCD block remap ("tile_order" m against the default) give the same bits"""
    B, H, Nq, Nk, D = dims
    q, k, v = plain_inputs(dev, dims, seed=76)
    run = lambda: K.attn_fwd(q, k, v, B, H, Nq, Nk, D, D ** -0.5)
    base = run()
    again = run()
    try:
        K.set_tile_order("m")
        other = run()
    finally:
        K.set_tile_order(K.DEFAULT_TILE_ORDER)
    for a, b_, c_ in zip(base, again, other):
        assert torch.equal(a, b_) and torch.equal(a, c_)


def case_contract(dev):
    """D = 520 (too wide) and D = 516 (not a multiple of 8) are refused with nothing written; the limits can be asked for; the
    backward keeps its limit of 160"""
    assert (K.attn_max_head_dim(), K.attn_max_head_dim(True)) == (512, 160)
    for D in (520, 516):
        q, k, v = (torch.zeros((16, D), dtype=f16, device=dev) for _ in range(3))
        o = torch.full((16, D), NAN, dtype=f16, device=dev)
        with pytest.raises(capi.CloraError):
            K.attn_fwd(q, k, v, 1, 1, 16, 16, D, D ** -0.5, out=o)
        assert bool(torch.isnan(o.float()).all())
    D = 256
    q, k, v, o, dO = (torch.zeros((16, D), dtype=f16, device=dev) for _ in range(5))
    lse = torch.zeros((1, 1, 16), dtype=f32, device=dev)
    with pytest.raises(capi.CloraError):
        K.attn_bwd(q, k, v, o, dO, lse, 1, 1, 16, 16, D, D ** -0.5, torch.empty_like(q), torch.empty_like(k), torch.empty_like(v))


def narrow_forward(dev):
    """the narrow shape whose bits must not move (D = 40: the kernels of clora_attn.hip)"""
    B, H, Nq, Nk, D = NARROW
    q, k, v = plain_inputs(dev, NARROW, seed=77)
    return K.attn_fwd(q, k, v, B, H, Nq, Nk, D, D ** -0.5)
