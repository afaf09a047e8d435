"""The cases of tests/kernel_cases.py that guard clora_ew.hip, clora_lora.hip, clora_norm.hip and the split-K finish of
clora_epilogue.h have teeth: the emulator library is rebuilt from a copy of the kernel sources with ONE small defect each
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

EW, NORM, LORA, EPI = "clora_ew.hip", "clora_norm.hip", "clora_lora.hip", "clora_epilogue.h"
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
}

_MSE_LOOP = "    EW_LOOP(i, n8) {\n        const half8 a = ld8(pred + i * 8), b = ld8(target + i * 8);\n        half8 o;\n#pragma unroll\n        for (int e = 0; e < 8; ++e) {\n            const float d = (float)a[e] - (float)b[e];\n            acc += d * d;"

# mutant -> (file, [(old, new)], the case that must fail on it, what its assertion message must match or None, a case that must still
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
}


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
    """one library per DISTINCT (file, edits): built side by side, the compiler runs outside the interpreter lock"""
    build_emu.build()                                   # the regular objects the mutant builds reuse
    builds = {}
    for name, (file_name, edits, *_rest) in MUTANTS.items():
        builds.setdefault((file_name, tuple(edits)), name)
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(8, len(os.sched_getaffinity(0))))) as pool:
        futs = {key: pool.submit(build_emu.build_mutant, str(tmp_path_factory.mktemp(name)), key[0], list(key[1])) for key, name in builds.items()}
        libs = {key: f.result() for key, f in futs.items()}
    return {name: libs[(file_name, tuple(edits))] for name, (file_name, edits, *_rest) in MUTANTS.items()}


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
