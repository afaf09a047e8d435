"""The GEMM tile table (include/clora.h clora_gemm_tile_t), pinned: the literal below is what the library's rows must say, and
every capability bit of a row is exercised on the kernel the row names.  Shared by tests/test_gemm_tiles_emu.py (emulator) and
tests/test_gemm_tiles_gpu.py (-m gpu); `dev` = "cpu" (emulator) or "cuda"."""
import math

import torch

from controllora_amd import capi, kernels as K
from tests import kernel_cases as KC

RING, V1, EIGHT, PATCH, WPATCH, STRIP = range(6)          # CLORA_TILE_*
G, D, L, C = 1, 2, 4, 8                                   # CLORA_TILE_CAP_*: GEGLU forward, lora_dpack, ln_out at N == BN, conv rows

# tile_cfg: (family, BM, BN, WM, WN, NST, BK, FLAGS, caps) -- written by hand from the tile's definition, never from the library
PINNED = {
    1: (RING, 128, 128, 2, 2, 3, 32, 0, G | C), 2: (RING, 128, 64, 4, 1, 3, 32, 0, C), 3: (RING, 64, 64, 2, 2, 3, 32, 0, C),
    4: (RING, 128, 128, 2, 2, 5, 32, 0, G | C), 5: (RING, 128, 64, 4, 1, 6, 32, 0, C), 6: (RING, 64, 64, 2, 2, 8, 32, 0, C),
    7: (RING, 256, 128, 2, 2, 3, 32, 0, G | C), 8: (RING, 256, 128, 2, 2, 3, 32, 1, G | C),
    9: (RING, 128, 128, 2, 2, 3, 32, 2, G | C),
    11: (V1, 128, 128, 2, 2, 3, 32, 0, C), 12: (V1, 128, 64, 4, 1, 3, 32, 0, C), 13: (V1, 64, 64, 2, 2, 3, 32, 0, C),
    21: (RING, 128, 128, 2, 2, 2, 64, 0, G | D | C), 22: (RING, 128, 64, 4, 1, 3, 64, 0, D | C),
    23: (RING, 64, 64, 2, 2, 3, 64, 0, D | C), 26: (RING, 128, 64, 4, 1, 2, 64, 0, D | C),
    31: (RING, 128, 128, 2, 2, 3, 32, 1, G | C), 32: (RING, 128, 64, 4, 1, 3, 32, 1, C), 33: (RING, 64, 64, 2, 2, 3, 32, 1, C),
    41: (RING, 128, 128, 2, 2, 2, 64, 1, G | D | C), 42: (RING, 128, 64, 4, 1, 3, 64, 1, D | C),
    43: (RING, 64, 64, 2, 2, 3, 64, 1, D | C),
    51: (RING, 128, 320, 4, 2, 2, 64, 0, D | L | C), 52: (RING, 64, 320, 2, 4, 3, 64, 0, D | L | C),
    53: (RING, 128, 256, 4, 2, 3, 64, 0, G | C),
    54: (RING, 128, 320, 4, 2, 2, 64, 1, D | L | C), 55: (RING, 64, 320, 2, 4, 3, 64, 1, D | L | C),
    56: (RING, 128, 256, 4, 2, 3, 64, 1, G | C),
    57: (RING, 256, 320, 4, 2, 2, 64, 1, C), 58: (RING, 256, 256, 4, 2, 2, 64, 1, G | C),
    59: (EIGHT, 256, 256, 2, 4, 0, 64, 0, G),             # 8 waves of 128x64; no ring depth, no FLAGS; a conv falls back to 58
    61: (STRIP, 0, 0, 0, 0, 0, 0, 0, 0),                  # no tile shape of its own; falls back to tile_cfg 0
    71: (PATCH, 256, 128, 4, 2, 3, 64, 0, 0), 72: (PATCH, 128, 128, 2, 4, 3, 64, 0, 0), 73: (PATCH, 128, 128, 4, 2, 3, 64, 0, 0),
    74: (PATCH, 256, 64, 8, 1, 4, 64, 0, 0), 75: (PATCH, 128, 64, 4, 2, 4, 64, 0, 0), 76: (PATCH, 128, 160, 4, 2, 3, 64, 0, 0),
    77: (WPATCH, 128, 128, 2, 4, 3, 64, 0, 0), 78: (WPATCH, 128, 64, 4, 2, 4, 64, 0, 0),
    79: (PATCH, 256, 160, 4, 2, 3, 64, 0, 0),             # patch rows: BM is the pixel count of the patch (256 for 71, 74, 79)
}
D_ROWS = sorted(c for c, r in PINNED.items() if r[8] & D)
L_ROWS = sorted(c for c, r in PINNED.items() if r[8] & L)
G_ROWS = sorted(c for c, r in PINNED.items() if r[8] & G)
PATCH_ROWS = sorted(c for c, r in PINNED.items() if r[0] in (PATCH, WPATCH))


def pinned_fused_down_tile(M, lora_seg, tile_cfg):
    """the replacement rule of a lora_dpack launch, as include/clora.h states it"""
    r = PINNED.get(tile_cfg)
    if r is not None and r[8] & D and lora_seg % r[2] == 0:
        return tile_cfg
    if lora_seg % 320 == 0:
        return 54 if M >= 32768 else 55
    return 43


def case_rows_are_the_pinned_table():
    rows = {c: (r.family, r.bm, r.bn, r.wm, r.wn, r.nst, r.bk, r.flags, r.caps) for c, r in K.gemm_tiles().items()}
    assert rows == PINNED, {c: (rows.get(c), PINNED.get(c)) for c in set(rows) | set(PINNED) if rows.get(c) != PINNED.get(c)}
    cdll, r, n = capi.lib().cdll, capi.GemmTile(), 0
    while cdll.clora_gemm_tile_at(n, r) == capi.OK:
        n += 1
    assert n == len(PINNED) and cdll.clora_gemm_tile_at(-1, r) == capi.ERR_ARG               # no row listed twice
    for cfg in range(-1, 100):
        rc = cdll.clora_gemm_tile_info(cfg, r)
        assert rc == (capi.OK if cfg in PINNED else capi.ERR_ARG) and (rc != capi.OK or r.tile_cfg == cfg), cfg
    assert cdll.clora_gemm_tile_info(1, None) == capi.ERR_ARG


def case_plain_launch_accepts_exactly_the_rows(dev):
    """a plain launch (two tiles of the smallest shape in each direction would not fit every tile: ONE ragged tile here, the sweeps of
    test_gemm_tile_configs cover several) runs on every row and on 0 = automatic; any other value in 0..99 is CLORA_ERR_ARG"""
    g = torch.Generator().manual_seed(7)
    M, N, Kd = 40, 24, 64
    A, B = KC.rnd((M, Kd), dev, g), KC.rnd((N, Kd), dev, g, 1 / math.sqrt(Kd))
    ref = A.float() @ B.float().T
    out = torch.empty((M, N), dtype=KC.f16, device=dev)
    for cfg in range(100):
        out.zero_()
        rc = capi.lib().cdll.clora_gemm_f16_ex(capi.ptr(A), Kd, capi.ptr(B), capi.ptr(out), N, M, N, Kd, None, None, 1, cfg, None, 0, capi.stream())
        assert rc == (capi.OK if cfg == 0 or cfg in PINNED else capi.ERR_ARG), (cfg, rc)
        if rc == capi.OK:
            assert KC.rel(out, ref) < 6e-4, cfg


def case_fused_down_rule():
    """clora_gemm_fused_down_tile == the pinned rule, for every tile_cfg value, segment widths that are / are not multiples of each
    BN, both sides of the M threshold"""
    for cfg in range(100):
        for seg in (64, 128, 192, 256, 320, 640, 960):
            for M in (150, 32767, 32768):
                assert K.fused_down_tile(M, seg, cfg) == pinned_fused_down_tile(M, seg, cfg), (cfg, seg, M)
    out = capi.C.c_int()
    assert capi.lib().cdll.clora_gemm_fused_down_tile(0, 64, 43, out) == capi.ERR_ARG
    assert capi.lib().cdll.clora_gemm_fused_down_tile(150, 64, 43, None) == capi.ERR_ARG


def case_d_row(dev, tile):
    """two column segments of exactly BN columns: the fused launch then runs on `tile` itself, and case_gemm_fused_down's fused-versus-
    unfused bit check proves that the BN of the row is the BN the kernel runs"""
    bn = PINNED[tile][2]
    assert K.fused_down_tile(150, bn, tile) == tile
    KC.case_gemm_fused_down(dev, M=150, N=2 * bn, K_=128, nseg=2, tile_cfg=tile)


def case_ln_bits(dev):
    for cfg in range(100):
        bn = PINNED[cfg][2] if cfg in L_ROWS else 320
        fus = capi.lib().cdll.clora_gemm_ln_fusable
        assert fus(150, bn, 64, cfg, 1) == (1 if cfg in L_ROWS else 0), cfg
        assert fus(150, bn + 64, 64, cfg, 1) == 0 and fus(150, bn, 64, cfg, 2) == 0, cfg


def case_patch_row(dev, tile):
    """the smallest eligible map runs on the patch kernel; a 4x4 map fits 128-pixel patches only (16 images of 6x6 exceed the 256-pixel
    tile's budget), 128-pixel rows fit the wide patch only: eligibility follows the row's BM and family"""
    fam, bm = PINNED[tile][0], PINNED[tile][1]
    if fam == WPATCH:
        KC.case_conv_patch(dev, 1, 3, 128, 128, 64, tile)
    elif bm == 128:
        KC.case_conv_patch(dev, 3, 8, 8, 128, 64, tile)
    else:
        KC.case_conv_patch(dev, 2, 16, 16, 128, 64, tile)
    small, _, _ = K.conv_fwd_desc(4, 4, 64, 3, 1, 1, kchunk=64)
    assert K.conv_patch_eligible(3 * 16, small, tile) == (bm == 128)
    wide, _, _ = K.conv_fwd_desc(2, 128, 64, 3, 1, 1, kchunk=64)
    assert K.conv_patch_eligible(256, wide, tile) == (fam == WPATCH)
    assert not K.conv_patch_eligible(256, wide, 21) and not K.conv_patch_eligible(256, wide, 0)
