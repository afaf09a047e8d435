"""The cases of tests/kernel_cases.py that guard clora_ew.hip, clora_lora.hip, clora_norm.hip, the split-K finish of
clora_epilogue.h and clora_gemm.hip have teeth: the emulator library is rebuilt from a copy of the kernel sources with ONE small defect each
(tests/hipemu/build_emu.build_mutant: the edited translation unit is recompiled, or every unit that includes an edited header), and
the case named beside the defect -- at the shape tests/test_kernels_emu.py runs it -- must fail on the mutant and pass on the real
sources.  Most defects sit on a path only a large enough launch takes: a second trip of a capped grid-stride loop, the unrolled
"N loads in flight" body of a fold (small shapes run its tail alone), a second row / column block, an accumulation into a buffer that
is not zero, a state slot the host writes.

clora_ew.hip
  ew_stride        EW_LOOP's stride doubled: every grid-stride loop skips its 2nd, 4th ... trip (caught by the elementwise case and, as
                   ew_stride_optimizer, by the loss / optimizer case on the same library)
  optim_world      optim_prep_kernel ignores state[11], the data-parallel world size
  adamw_lr_mult    adamw_kernel ignores state[10], the device-resident LR multiplier
  colsum_rows      colsum_kernel: every row block after the first starts 4 rows late
  mse_stride       mse_kernel alone strides twice its grid (its grid is capped at 256 blocks, not 4096)
  copy2d_row       copy2d_kernel reads source rows modulo 32768
clora_norm.hip
  gn_params_v0     gn_bwd_params_block: the 8-loads-in-flight loop adds v0[0] / v1[0] eight times
  gn_params_slot   the same loop loads its seventh partial twice and never its eighth
clora_lora.hip
  wgrad_overwrite  lora_wgrad_finish_kernel stores instead of accumulating into the caller's gradient
  wgrad_finish_v0  lora_wgrad_finish_kernel: the unrolled slab loop adds v[0] eight times (single job, and as wgrad_finish_v0_multi the
                   launch whose jobs differ in size)
  lora_up_stride   lora_up_kernel strides twice its grid
  wgrad_col_block  lora_wgrad_kernel: column blocks after the first load column 0
  up_tr_u0         (control: caught before this module existed) lora_up's transposed-U path reads u0 twice
  down_r2          (control) lora_down drops the row limit r2 of the second input
clora_epilogue.h
  finish_b0        finish_chunk8: the 4-slabs-in-flight loop adds b[0] for every slab of the group
  finish_tail      finish_chunk8: the tail after a full group reads slab 4 for every later slab (columns 4..7)

clora_gemm.hip (the first five survived every CPU test before their killing cases existed; patch_clamp is a survivor found here)
  wgrad_dy_tile    conv_wgrad_kernel reads dY column ncol & 63: every output-channel tile after the first re-reads channels 0..63
  finish_stride    splitk_finish_kernel strides twice its grid (capped at 2048 blocks: a second trip needs M * N / 8 > 524,288)
  unpack_stride    conv_wgrad_unpack_kernel strides twice its grid (same cap: Co * 9 * Cip > 524,288)
  pack_stride      conv_weight_pack_kernel strides twice its grid (same cap)
  strip_halo       conv3x3_strip_kernel treats the row above its row chunk as zero padding (yy >= y_beg instead of yy >= 0): every
                   CPU shape had H <= 8 = one chunk; strip8_halo the same in conv3x3_strip8_kernel, wgrad_patch_halo in
                   conv_wgrad_patch_kernel (its row-chunk walk: chunks of at least 4 rows, caught since H = 5 was a case)
  patch_clamp      conv3x3_patch_kernel: a split whose slab range is clamped to the slab count does nothing.  SURVIVOR: the CPU shapes
                   had 1 or 2 slabs of 64 channels, which every split count divides; 192 channels in two splits (2 + 1 slabs) close it
  partial_slab     dma_epilogue stores the partial sums of split z into slab z & 1
  wgrad_nst        conv_wgrad_kernel drops the ragged last 64-row stage of an M block (nst rounds down)
  wgrad_mrow       conv_wgrad_kernel: every M block after the first starts 64 rows late
  oihw_scatter     conv_wgrad_kernel's OIHW scatter swaps ky and kx
  tiles_k          (control: caught before) the launch of conv_wgrad_kernel counts its k tiles without the bias column
clora_ew.hip, multi-job forms of the two copies (grid.x capped at 1024 blocks per job)
  pack_multi_stride / unpack_multi_stride   the kernels stride twice their grid

Defects of clora_gemm.hip in DIFFERENT kernels share one library where neither's killing case runs the other's defective path (GROUPS
below: four compilations of the largest translation unit instead of thirteen); each was also built alone once and failed the same
case.  The assertion message names the output that is wrong wherever the case has one.

Not in the table because it changes nothing: the strip kernels' `live ? y : y_beg` row address -- a row that is not live always reads
the zero page, the address is never used.  Not expressible on the emulator: the order in which the fp32 atomics of the two
weight-gradient kernels retire (blocks run one after the other: one summation order), and every wait count / barrier placement of
the DMA rings beyond what tests/test_emu_async_model.py models.

Not in the table, because no mutant can express it here: grad_sumsq_kernel's former one-fp32-atomic-per-block sum (the gradient norm
followed the order in which blocks retired).  The emulator runs the blocks of a launch one after the other, so that kernel gives the
same bits on every launch; tests/kernel_cases.py::case_grad_sumsq_reproducible fails on it on the GPU only (4 and 9 different norms in
15 launches on an MI355X)."""
import concurrent.futures
import contextlib
import glob
import os

import pytest

from controllora_amd import capi
from tests import kernel_cases as KC
from tests.hipemu import build_emu

EW, NORM, LORA, EPI, GEMM = "clora_ew.hip", "clora_norm.hip", "clora_lora.hip", "clora_epilogue.h", "clora_gemm.hip"
BIG = 4096 * 256 + 300

# the cases, by the name the table below uses (shapes = those of tests/test_kernels_emu.py)
CASES = {
    "optimizer": lambda: KC.case_loss_and_optimizer("cpu"),
    "optimizer_past_cap": lambda: KC.case_loss_and_optimizer("cpu", n=BIG),
    "elementwise_past_cap": lambda: KC.case_elementwise_past_cap("cpu"),
    "copies_past_cap": lambda: KC.case_copies_past_cap("cpu"),
    "copies_small": lambda: KC.case_elementwise("cpu"),
    "colsum": lambda: KC.case_colsum("cpu", 1030, 130),
    "colsum_one_block": lambda: KC.case_colsum("cpu", 37, 8),
    "groupnorm_72_partials": lambda: KC.case_groupnorm("cpu", 2, 2300, 64, 8, True, train_params=True),
    "groupnorm_few_partials": lambda: KC.case_groupnorm("cpu", 2, 64, 32, 32, True, train_params=True),
    "lora_small": lambda: KC.case_lora("cpu", 128, 72, 40, 8, x_rows=32),
    "lora_300": lambda: KC.case_lora("cpu", 300, 320, 64, 4),
    "lora_34_slabs": lambda: KC.case_lora("cpu", 2113, 72, 520, 4),
    "lora_up_past_cap": lambda: KC.case_lora("cpu", 8200, 72, 1032, 4),
    "wgrad_multi": lambda: KC.case_lora_wgrad_multi("cpu"),
    "rank_control": lambda: KC.case_rank_control("cpu"),
    "lora_down_mode0": lambda: KC.case_lora_down_mode("cpu", 0, 200, 136),
    "gemm_split3": lambda: KC.case_gemm_plain("cpu", 256, 640, 320, 3),
    "gemm_split4": lambda: KC.case_gemm_plain("cpu", 256, 136, 512, 4),
    "gemm_split6": lambda: KC.case_gemm_plain("cpu", 256, 136, 768, 6),
    "gemm_split2": lambda: KC.case_gemm_plain("cpu", 520, 136, 160, 2),
    "gemm_finish_past_cap": lambda: KC.case_gemm_plain("cpu", 4104, 1032, 64, 2),
    "pack_unpack_past_cap": lambda: KC.case_conv_pack_unpack_past_cap("cpu"),
    "pack_unpack_multi_past_cap": lambda: KC.case_conv_pack_unpack_past_cap("cpu", ((229, 253, 256), (16, 3, 8), (64, 32, 32))),
    "conv_padded": lambda: KC.case_conv_padded_channels("cpu"),
    "conv_one_tile": lambda: KC.case_conv("cpu", 1, 8, 8, 16, 24),
    "conv_two_tiles": lambda: KC.case_conv("cpu", 1, 8, 8, 16, 72),
    "conv_240_rows": lambda: KC.case_conv("cpu", 2, 12, 10, 16, 24),
    "conv_64_channels": lambda: KC.case_conv("cpu", 2, 4, 4, 64, 32),
    "conv_upsampled": lambda: KC.case_conv("cpu", 2, 12, 10, 16, 24, ups=True),
    "strip_one_chunk": lambda: KC.case_conv_strip("cpu", 1, 3, 128, 32, 32),
    "strip_three_chunks": lambda: KC.case_conv_strip("cpu", 1, 17, 128, 32, 32),
    "strip8_one_chunk": lambda: KC.case_conv_strip("cpu", 2, 3, 128, 8, 32),
    "strip8_three_chunks": lambda: KC.case_conv_strip("cpu", 2, 17, 128, 8, 32),
    "wgrad_patch_one_chunk": lambda: KC.case_conv_wgrad_patch("cpu", 1, 3, 128, 32, 32),
    "wgrad_patch_256_rows": lambda: KC.case_conv_wgrad_patch("cpu", 1, 2, 128, 32, 64),
    "wgrad_patch_two_chunks": lambda: KC.case_conv_wgrad_patch("cpu", 2, 5, 64, 32, 64),
    "patch_two_slabs": lambda: KC.case_conv_patch("cpu", 2, 8, 8, 128, 64, 72),
    "patch_three_slabs": lambda: KC.case_conv_patch("cpu", 1, 8, 8, 192, 64, 72),
}

_MSE_LOOP = "    EW_LOOP(i, n8) {\n        const half8 a = ld8(pred + i * 8), b = ld8(target + i * 8);\n        half8 o;\n#pragma unroll\n        for (int e = 0; e < 8; ++e) {\n            const float d = (float)a[e] - (float)b[e];\n            acc += d * d;"

_HALO = "if (yy >= 0 && yy < p.H) src = p.X + (ptrdiff_t)row * CIN + soff[j];"      # conv_wgrad_patch_kernel, conv3x3_strip_kernel, conv3x3_strip8_kernel
_HALO_CHUNK = "if (yy >= y_beg && yy < p.H) src = p.X + (ptrdiff_t)row * CIN + soff[j];"

# mutant -> (file, [(old, new)] or [(old, new, occurrence)], the case that must fail on it, what its assertion message must match or None, a case that must still
# pass on the mutant library or None: the defect is confined to the path the killing case reaches)
MUTANTS = {
    "ew_stride": (EW, [("i += (size_t)gridDim.x * 256)", "i += (size_t)gridDim.x * 512)")], "elementwise_past_cap", r"add", "copies_small"),
    "ew_stride_optimizer": (EW, [("i += (size_t)gridDim.x * 256)", "i += (size_t)gridDim.x * 512)")], "optimizer_past_cap", None, "optimizer"),
    "optim_world": (EW, [("const float inv = 1.0f / (st[3] * (st[11] > 0.f ? st[11] : 1.0f));", "const float inv = 1.0f / st[3];")],
                    "optimizer", r"world size 2", None),
    "adamw_lr_mult": (EW, [("lr *= (st[10] > 0.f ? st[10] : 1.0f);", "lr *= 1.0f;")], "optimizer", r"lr multiplier 0\.5", None),
    "colsum_rows": (EW, [("for (int m = m_beg + w; m < m_end; m += 4) {", "for (int m = m_beg + w + (blockIdx.y ? 4 : 0); m < m_end; m += 4) {")],
                    "colsum", None, "colsum_one_block"),
    "mse_stride": (EW, [(_MSE_LOOP, _MSE_LOOP.replace("EW_LOOP(i, n8) {", "for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; "
                                                                             "i += (size_t)gridDim.x * 512) {"))],
                   "optimizer_past_cap", None, "optimizer"),
    "copy2d_row": (EW, [("st8(dst + m * ldd + n, ld8(src + m * lds + n));", "st8(dst + m * ldd + n, ld8(src + (m & 32767) * lds + n));")],
                   "copies_past_cap", r"concat", "copies_small"),
    "gn_params_v0": (NORM, [("for (int u = 0; u < 8; ++u) { sa += v0[u]; sb += v1[u]; }", "for (int u = 0; u < 8; ++u) { sa += v0[0]; sb += v1[0]; }")],
                     "groupnorm_72_partials", None, "groupnorm_few_partials"),
    "gn_params_slot": (NORM, [("const float* pp = p.chpart + ((size_t)(i + 8 * u) * p.C + c) * 2; v0[u] = pp[0]; v1[u] = pp[1];",
                               "const float* pp = p.chpart + ((size_t)(i + 8 * (u < 7 ? u : 6)) * p.C + c) * 2; v0[u] = pp[0]; v1[u] = pp[1];")],
                       "groupnorm_72_partials", None, "groupnorm_few_partials"),
    "wgrad_overwrite": (LORA, [("*dst += p.scale * s;", "*dst = p.scale * s;")], "lora_small", None, None),
    "wgrad_finish_v0": (LORA, [("for (int u = 0; u < 8; ++u) s += v[u];", "for (int u = 0; u < 8; ++u) s += v[0];")], "lora_34_slabs", None, "lora_300"),
    "wgrad_finish_v0_multi": (LORA, [("for (int u = 0; u < 8; ++u) s += v[u];", "for (int u = 0; u < 8; ++u) s += v[0];")], "wgrad_multi", None, None),
    "lora_up_stride": (LORA, [("i < total; i += (size_t)gridDim.x * 256) {\n        const size_t m = i / NC;\n        const int n = (int)(i - m * NC) * 8;\n        const float* tr",
                               "i < total; i += (size_t)gridDim.x * 512) {\n        const size_t m = i / NC;\n        const int n = (int)(i - m * NC) * 8;\n        const float* tr")],
                       "lora_up_past_cap", None, "lora_300"),
    "wgrad_col_block": (LORA, [("const int nc = nok ? n : 0;", "const int nc = (nok && n < 512) ? n : 0;")], "lora_34_slabs", None, "lora_300"),
    "up_tr_u0": (LORA, [("const floatx4 u1 = *reinterpret_cast<const floatx4*>(p.U + (size_t)j * p.ldu + n + 4);",
                         "const floatx4 u1 = *reinterpret_cast<const floatx4*>(p.U + (size_t)j * p.ldu + n);")], "rank_control", None, "lora_300"),
    "down_r2": (LORA, [("if (p.r2 > 0) jok = li < p.r2;", "if (false) jok = li < p.r2;")], "lora_down_mode0", None, "lora_300"),
    "finish_b0": (EPI, [("for (int e = 0; e < 4; ++e) { s[e] += a[u][e]; s[4 + e] += b[u][e]; }", "for (int e = 0; e < 4; ++e) { s[e] += a[u][e]; s[4 + e] += b[0][e]; }")],
                  "gemm_split4", None, "gemm_split3"),
    "finish_tail": (EPI, [("const floatx4 b = *reinterpret_cast<const floatx4*>(q0 + (size_t)z * zs + 4);",
                           "const floatx4 b = *reinterpret_cast<const floatx4*>(q0 + (size_t)(z > 4 ? 4 : z) * zs + 4);")],
                    "gemm_split6", None, "gemm_split4"),
    "wgrad_dy_tile": (GEMM, [("p.dY + (size_t)mrow * p.ldy + ncol[q] : zero_page;", "p.dY + (size_t)mrow * p.ldy + (ncol[q] & 63) : zero_page;")],
                      "conv_two_tiles", None, "conv_one_tile"),
    "finish_stride": (GEMM, [("c < chunks; c += (size_t)gridDim.x * 256)", "c < chunks; c += (size_t)gridDim.x * 512)")],
                      "gemm_finish_past_cap", None, "gemm_split3"),
    "unpack_stride": (GEMM, [("i < nw + (gb ? Co : 0); i += gridDim.x * 256)", "i < nw + (gb ? Co : 0); i += gridDim.x * 512)")],
                      "pack_unpack_past_cap", r"'unpack ", "conv_padded"),
    "pack_stride": (GEMM, [("i < nf + nd; i += gridDim.x * 256)", "i < nf + nd; i += gridDim.x * 512)")], "pack_unpack_past_cap", r"'pack ", "conv_padded"),
    "wgrad_patch_halo": (GEMM, [(_HALO, _HALO_CHUNK, 0)], "wgrad_patch_two_chunks", None, "wgrad_patch_one_chunk"),
    "strip_halo": (GEMM, [(_HALO, _HALO_CHUNK, 1)], "strip_three_chunks", None, "strip_one_chunk"),
    "strip8_halo": (GEMM, [(_HALO, _HALO_CHUNK, 2)], "strip8_three_chunks", None, "strip8_one_chunk"),
    "patch_clamp": (GEMM, [("const int cs_end = cs_end_ < slabs ? cs_end_ : slabs;", "const int cs_end = cs_end_ <= slabs ? cs_end_ : cs_beg;")],
                    "patch_three_slabs", None, "patch_two_slabs"),
    "partial_slab": (GEMM, [("const int wm = w / WN, wn = w % WN;\n    if (p.partial) {\n        float* slab = p.partial + (size_t)split * p.M * p.N;",
                             "const int wm = w / WN, wn = w % WN;\n    if (p.partial) {\n        float* slab = p.partial + (size_t)(split & 1) * p.M * p.N;")],
                     "gemm_split3", None, "gemm_split2"),
    "wgrad_nst": (GEMM, [("const int nst = (mend - mbeg + BMR - 1) / BMR;", "const int nst = (mend - mbeg) / BMR;")], "conv_240_rows", None, "conv_one_tile"),
    "wgrad_mrow": (GEMM, [("int mrow = mbeg + lm;", "int mrow = mbeg + (blockIdx.y ? BMR : 0) + lm;")], "wgrad_patch_one_chunk", None, "wgrad_patch_256_rows"),
    "oihw_scatter": (GEMM, [("atomicAdd(p.dW + ((size_t)n * p.oihw_ci + ci) * taps + tap, acc[i][j][r]);",
                             "atomicAdd(p.dW + ((size_t)n * p.oihw_ci + ci) * taps + (taps == 9 ? (tap % 3) * 3 + tap / 3 : tap), acc[i][j][r]);")],
                     "conv_one_tile", None, "conv_upsampled"),
    "tiles_k": (GEMM, [("a.tiles_k = clora_cdiv(K + (db ? 8 : 0), 64);", "a.tiles_k = clora_cdiv(K, 64);")], "conv_64_channels", None, "conv_upsampled"),
    "pack_multi_stride": (EW, [("i < nf + nd; i += gridDim.x * 256)", "i < nf + nd; i += gridDim.x * 512)")],
                          "pack_unpack_multi_past_cap", r"multi-job pack", "conv_padded"),
    "unpack_multi_stride": (EW, [("i < nw + (p.grad_b ? Co : 0); i += gridDim.x * 256)", "i < nw + (p.grad_b ? Co : 0); i += gridDim.x * 512)")],
                            "pack_unpack_multi_past_cap", r"multi-job unpack", "conv_padded"),
}

# defects that share one compilation: different kernels of one file, and no killing / control case of one runs the defective path of
# another (a capped-stride defect is inert below its cap; the halo defects are inert in a one-chunk launch; see the module docstring).
# The edits of a group are applied in the order listed: an occurrence number counts what is left of the anchor at that point.
GROUPS = [("wgrad_dy_tile", "finish_stride", "unpack_stride", "strip_halo", "patch_clamp", "wgrad_patch_halo"),
          ("pack_stride", "wgrad_nst", "strip8_halo"),
          ("wgrad_mrow", "partial_slab"),
          ("oihw_scatter", "tiles_k")]


@contextlib.contextmanager
def _use(lib_path):
    old = capi._LIB
    capi._LIB = capi.Lib(lib_path, require_device=False)
    try:
        yield
    finally:
        capi._LIB = old


@pytest.fixture(scope="module")
def mutant_libs(tmp_path_factory):
    """one library per DISTINCT (file, edits) or per group of GROUPS: built side by side, the compiler runs outside the interpreter lock"""
    build_emu.build()                                   # the regular objects the mutant builds reuse
    builds, member = {}, {}
    for group in GROUPS:
        files = {MUTANTS[name][0] for name in group}
        assert len(files) == 1, group
        key = (files.pop(), tuple(e for name in group for e in MUTANTS[name][1]))
        builds[key] = group[0]
        member.update({name: key for name in group})
    for name, (file_name, edits, *_rest) in MUTANTS.items():
        if name not in member:
            member[name] = (file_name, tuple(edits))
            builds.setdefault(member[name], name)
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(8, len(os.sched_getaffinity(0))))) as pool:
        futs = {key: pool.submit(build_emu.build_mutant, str(tmp_path_factory.mktemp(name)), key[0], list(key[1])) for key, name in builds.items()}
        libs = {key: f.result() for key, f in futs.items()}
    return {name: libs[key] for name, key in member.items()}


_passed_on_real_sources = set()


def _real_sources_pass(case):
    if case not in _passed_on_real_sources:             # several mutants share a case: the unmodified sources run it once
        with _use(build_emu.build()):
            CASES[case]()
        _passed_on_real_sources.add(case)


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_kernel_mutant_is_caught(name, mutant_libs):
    _, _, fails, what, still_passes = MUTANTS[name]
    _real_sources_pass(fails)                           # the unmodified sources pass the very case ...
    with _use(mutant_libs[name]):
        with pytest.raises(AssertionError, match=what):
            CASES[fails]()                              # ... that the defect fails
        if still_passes is not None:
            CASES[still_passes]()                       # and the defect sits on the path only the killing case reaches


def test_header_mutation_reaches_every_including_unit():
    """build_mutant's include scan: an edited header rebuilds exactly the translation units whose text includes it, directly or through
    another header; an edited .hip rebuilds itself alone"""
    units = lambda f: build_emu.units_including(build_emu.CSRC, f)
    assert units("clora_epilogue.h") == {"clora_gemm.hip", "clora_norm.hip"}
    assert units("clora_attn_common.h") == {"clora_attn.hip", "clora_attn_wide.hip"}
    assert units("clora_common.h") == {os.path.basename(p) for p in glob.glob(os.path.join(build_emu.CSRC, "*.hip"))}
    assert units("clora_lora.hip") == {"clora_lora.hip"}
    assert units("no_such_header.h") == set()
