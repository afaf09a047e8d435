"""The attention cases of tests/kernel_cases.py have teeth: the emulator library is rebuilt from a copy of the kernel sources with ONE
small defect each in clora_attn.hip (tests/hipemu/build_emu.build_mutant: only that translation unit is recompiled), and the case that
guards the mutated line must fail on the mutant -- with a message that names the wrong output -- and pass on the real sources; a
control case beside it passes on the mutant library: the defect sits on the path only the killing case reaches.  The mutants of
clora_attn_wide.hip are in tests/test_attention_wide_emu.py.

forward
  causal_mask      the causal mask hides the diagonal (`>=` for `>`): row 0 sees no key at all              -> case_attention_causal
  lse_units        the LSE is stored in base 2 (the conversion `* kLn2` dropped)                            -> case_attention_full, LSE bound
  ld_v_as_k_fwd    the first V tile is fetched with K's row stride                                          -> case_attention_strides, o
  fwd_rebase_l     a rebase after the first tile does not rescale the running sum (`lrun[qg] *= alpha`)     -> peaked softmax at D = 64, o
  fwd_rebase_qg    the rebase condition of query group 0 is used for both groups                            -> the same case, o
dQ
  ld_v_as_k_dq     the V tiles after the first are fetched with K's row stride                              -> case_attention_strides, dq
  ld_do_as_o_dq    the dO fragment is read with o's row stride                                              -> case_attention_strides, dq
  ld_o_as_q_delta  the delta prologue reads o with q's row stride                                           -> case_attention_strides, dq
  dq_mask          the keys a ragged last tile does not have are not masked                                 -> case_attention_negative_logits
dK/dV
  wide_dkv_row     the 8-wave kernel -- and only it -- skips the last key row of a ragged block             -> case_attention_full under
                   "attn_bwd_waves" 8, while the 4-wave kernels of the same library still pass
  ld_v_as_k_dkv    the V fragment is read with K's row stride                                               -> case_attention_strides, dk
  ld_do_as_q_dkv   the dO tiles after the first are fetched with q's row stride                             -> case_attention_strides, dk
  ld_dv_as_dk      the unsplit kernel stores dV with dK's row stride                                        -> case_attention_strides, dv
  split_last       the last query split is one row short                                                    -> three splits at D = 64, dk
  split_slab_dt    the split epilogue stores d-tile 3 of dV for every later d-tile                          -> three splits at D = 80
                   (D = 64 has four d-tiles: passes)
the fold of the split slabs (attn_dkv_convert_kernel) and the split rule
  ld_dv_as_dk_convert  dV is stored with dK's row stride                                                    -> case_attention_strides, 3 splits
  convert_u0       the unrolled group of four adds dV's first slab four times                               -> five splits (three: passes)
  convert_tail     the tail after a full group reads slab 4 for every later slab                            -> six splits (five: passes)
  convert_stride   the kernel strides twice its grid (capped at 2048 blocks: a second trip needs B * Nk * H * D > 2,097,152)
                                                                                                            -> (1, 14, 512, 1024, 160)
  ws_clamp         the split count ignores workspace_bytes                                                  -> case_attention_workspace: the
                   bytes past the stated budget lose their sentinel (they lie in the case's own, larger buffer: nothing is stored outside
                   allocated memory)

Before the cases named here existed, ten of these survived every attention case of the suite: every case gave k and v, o and dO, and
dq, dk and dv equal row strides (the seven stride swaps, wide_ld_v_as_k of the wide kernel among them), the split path ran at D = 40
and 64 only, with 3 and 5 splits, and never past the fold's grid cap.  Seven more (convert_u0, split_last, ld_do_as_q_dkv,
ld_o_as_q_delta, fwd_rebase_l, fwd_rebase_qg, dq_mask) failed one to three cases of the norm-only, fp32-referenced case_attention family; all but dq_mask are bound
to an fp64 case here.  dq_mask cannot be: an unmasked missing key is a zero row of K, so its dS only reaches dq as 0 * dS, which
shows only where dS overflows -- exp2(-LSE * log2 e) = inf, an LSE below -88.  Logits that low are rounded (the scaled operand is fp16:
2^-12 relative per term) to 1 % of P and worse, which no input passes the 4e-3 limits with; case_attention_negative_logits asserts
what can be asserted there, that every gradient is finite.

No stride mutant stores outside the buffers of case_attention_strides (each holds two rows more than its row count at the largest of
the eight strides).  Defects in DIFFERENT kernels share one compilation where no killing or control case of one runs the defective
path of another (GROUPS; the libraries are built side by side).

Not in the table because nothing can kill them (equivalent; both were built and run against every attention case):
  the -1.0e30f padding of load_ld in the dK/dV kernel: padded Q and dO rows are zero rows, their contribution is 0 whatever P is;
  the 1.0e30f of Lq for queries past Nq in the dQ kernel: those columns are never stored.
Not observable by any fp16-level check: a 1 % error on one key in 64 of dS from the third tile on -- below one fp16 rounding of dq.

Emulator run times measured on an 8-CPU machine.  This module: 54 s, of which the eight side-by-side builds take 7 s and convert_stride
37 s ((1, 14, 512, 1024, 160) on the real sources and on the mutant; every other mutant under 2.1 s).  The cases added to
tests/test_kernels_emu.py with these mutants: 29 s for the 20 of them, of which that shape takes 20.7 s (it stays an emulator case: one
minute was the limit set for it), the workspace case 1.2 s and every other at most 0.75 s; all 177 attention cases of that module 51 s.
tests/test_attention_wide_emu.py: 7 s for its 17 tests, the stride case 0.1 s, its two mutant builds 0.6 s, each wide mutant under 0.7 s."""
import concurrent.futures
import contextlib
import os

import pytest

from controllora_amd import capi
from tests import kernel_cases as KC
from tests.hipemu import build_emu

ATTN = "clora_attn.hip"


def _waves8(waves):
    def run():
        with KC.options(attn_bwd_waves=waves):
            KC.case_attention_full("cpu", 1, 2, 270, 130, 40, strided=True)
    return run


# the cases, by the name the table below uses (shapes = those of tests/test_kernels_emu.py)
CASES = {
    "causal": lambda: KC.case_attention_causal("cpu", 2, 2, 77, 64),
    "full": lambda: KC.case_attention_full("cpu", 1, 2, 70, 150, 40),
    "full_8_waves": _waves8(8),
    "full_4_waves": _waves8(4),
    "peaked_64": lambda: KC.case_attention_full("cpu", 1, 2, 70, 150, 64, q_scale=6.0),
    "full_64": lambda: KC.case_attention_full("cpu", 1, 2, 70, 150, 64),
    "strides": lambda: KC.case_attention_strides("cpu", 2, 2, 70, 150, 40),
    "strides_split": lambda: KC.case_attention_strides("cpu", 2, 2, 513, 77, 40),
    "negative_ragged": lambda: KC.case_attention_negative_logits("cpu", 1, 2, 40, 40, 40),
    "negative_whole_tile": lambda: KC.case_attention_negative_logits("cpu", 1, 2, 40, 64, 64),
    "split3_40": lambda: KC.case_attention_split("cpu", 2, 2, 513, 77, 40, splits=3),
    "split3_64": lambda: KC.case_attention_split("cpu", 2, 2, 513, 77, 64, splits=3),
    "split3_80": lambda: KC.case_attention_split("cpu", 2, 2, 513, 77, 80, splits=3),
    "split5": lambda: KC.case_attention_split("cpu", 1, 2, 640, 77, 40, splits=5),
    "split6": lambda: KC.case_attention_split("cpu", 1, 1, 1100, 77, 40, splits=6, strided=False, tail=True),
    "fold_past_cap": lambda: KC.case_attention_split("cpu", 1, 14, 512, 1024, 160, splits=4),
    "workspace": lambda: KC.case_attention_workspace("cpu", 2, 2, 1100, 77, 40),
}

_V_NEXT = "dma.template issue<false>(vbase + (size_t)(kv0 + BKV) * p.ldv, p.ldv, nrows, nb + BKV * LDK, w);"
_DO_NEXT = "dma.template issue<false>(dobase + (size_t)(qq + BQT) * p.lddo, p.lddo, nrows, nb + BQT * LDK, w);"

# mutant -> ([(old, new)] of clora_attn.hip, the case that must fail on it, what its assertion message must match or None, a case that must
# still pass on the mutant library or None)
MUTANTS = {
    "causal_mask": ([("if (kl >= rows || key > q0 + li) s[kt][0][r] = kNegBig;", "if (kl >= rows || key >= q0 + li) s[kt][0][r] = kNegBig;"),
                     ("if (kl >= rows || key > q0 + 16 + li) s[kt][1][r] = kNegBig;", "if (kl >= rows || key >= q0 + 16 + li) s[kt][1][r] = kNegBig;")],
                    "causal", None, None),
    "lse_units": ([("= (mref[qg] + log2f(lt)) * kLn2;", "= (mref[qg] + log2f(lt));")], "full", r"\('lse', ", None),
    "wide_dkv_row": ([("        if (key < p.Nk) {\n", "        if (key < p.Nk && !(NWV == 8 && key == p.Nk - 1)) {\n")],
                     "full_8_waves", r"\('dk', ", "full_4_waves"),
    "ld_v_as_k_fwd": ([("dv_.template issue<ONES>(vbase, p.ldv, rows0, smem + BKV * LDK, w);",
                        "dv_.template issue<ONES>(vbase, p.ldk, rows0, smem + BKV * LDK, w);")], "strides", r"\('o', ", "full"),
    "ld_v_as_k_dq": ([(_V_NEXT, _V_NEXT.replace("p.ldv, nrows", "p.ldk, nrows"))], "strides", r"\('dq', ", "full"),
    "ld_v_as_k_dkv": ([("vf[kg][ks] = ok ? ld8(p.v + ((size_t)b * p.Nk + key) * p.ldv + h * D + d) : zero8();",
                        "vf[kg][ks] = ok ? ld8(p.v + ((size_t)b * p.Nk + key) * p.ldk + h * D + d) : zero8();")], "strides", r"\('dk', ", "full"),
    "ld_do_as_o_dq": ([("dof[qg][ks] = ok ? ld8(p.dO + ((size_t)b * p.Nq + q) * p.lddo + h * D + d) : zero8();",
                        "dof[qg][ks] = ok ? ld8(p.dO + ((size_t)b * p.Nq + q) * p.ldo + h * D + d) : zero8();")], "strides", r"\('dq', ", "full"),
    "ld_o_as_q_delta": ([("const half8 ov = ld8(p.o + ((size_t)b * p.Nq + q) * p.ldo + h * D + d);",
                          "const half8 ov = ld8(p.o + ((size_t)b * p.Nq + q) * p.ldq + h * D + d);")], "strides", r"\('dq', ", "full"),
    "ld_do_as_q_dkv": ([(_DO_NEXT, _DO_NEXT.replace("p.lddo, nrows", "p.ldq, nrows"))], "strides", r"\('dk', ", "full"),
    "ld_dv_as_dk": ([("st4(p.dv + ((size_t)b * p.Nk + key) * p.lddv + h * D + d, ov);", "st4(p.dv + ((size_t)b * p.Nk + key) * p.lddk + h * D + d, ov);")],
                    "strides", r"\('dv', ", "full"),
    "ld_dv_as_dk_convert": ([("st4(p.dv + row * p.lddv + c, va);", "st4(p.dv + row * p.lddk + c, va);")], "strides_split", r"\('dv', ", "full"),
    "split_slab_dt": ([("*reinterpret_cast<floatx4*>(dst + plane) = dvacc[dt][kg];", "*reinterpret_cast<floatx4*>(dst + plane) = dvacc[dt > 3 ? 3 : dt][kg];")],
                      "split3_80", r"\('dv', ", "split3_64"),
    "convert_tail": ([("const float* q = q0 + (size_t)z * 2 * plane;", "const float* q = q0 + (size_t)(z > 4 ? 4 : z) * 2 * plane;")],
                     "split6", r"\('dk', ", "split5"),
    "convert_stride": ([("i < total; i += (size_t)gridDim.x * 256)", "i < total; i += (size_t)gridDim.x * 512)")],
                       "fold_past_cap", r"\('dk', 'not every element was written'\)", "split3_64"),
    "convert_u0": ([("for (int u = 0; u < 4; ++u) { a += ta[u]; bb += tb[u]; }", "for (int u = 0; u < 4; ++u) { a += ta[u]; bb += tb[0]; }")],
                   "split5", r"\('dv', ", "split3_40"),
    "split_last": ([("const int q_end = (q_beg + p.q_per_split < p.Nq) ? q_beg + p.q_per_split : p.Nq;",
                     "const int q_end = (q_beg + p.q_per_split < p.Nq) ? q_beg + p.q_per_split : p.Nq - (blockIdx.z > 0 ? 1 : 0);")],
                   "split3_64", r"\('dk', ", "full"),
    "fwd_rebase_l": ([("lrun[qg] *= alpha;", "lrun[qg] *= 1.f;")], "peaked_64", r"\('o', ", "full_64"),
    "fwd_rebase_qg": ([("const float d = (first || mx[qg] > kRebase) ? mx[qg] : 0.f;", "const float d = (first || mx[0] > kRebase) ? mx[qg] : 0.f;")],
                      "peaked_64", r"\('o', ", "full_64"),
    "dq_mask": ([("const bool ok = (kt * 16 + 4 * g + r) < rows;", "const bool ok = true;")], "negative_ragged", r"\('dq', ", "negative_whole_tile"),
    "ws_clamp": ([("if (workspace && ns > (int)(workspace_bytes / slab)) ns = (int)(workspace_bytes / slab);", "")],
                 "workspace", r"\('workspace', '\d+ bytes past", "split3_64"),
}

# defects that share one compilation: each sits in a different kernel (or on a path of its own: the causal instantiation, the unsplit and
# the split store, a split count, a head size), and none is reached by the killing or the control case of another member:
#   the stride swaps do nothing where the swapped strides are equal (every case but case_attention_strides); one per group, except the
#     two dV stores, of which the unsplit kernel has one and the fold kernel the other
#   lse_units spoils every unmasked forward and goes with the causal mutant alone (the causal entry point stores no LSE)
#   the rebase mutants need a peaked softmax, dq_mask an LSE below -88, wide_dkv_row the forced 8-wave kernel, split_slab_dt splits at
#     D > 64, convert_u0 four splits or more (so not with ws_clamp, which turns two splits into six), convert_tail six,
#     convert_stride and ws_clamp their one shape each ((1, 14, 512, 1024, 160) splits four ways at D = 160: neither split_slab_dt, convert_u0 nor
#     split_last go with convert_stride)
GROUPS = [("causal_mask", "lse_units"),
          ("ld_v_as_k_fwd", "split_slab_dt", "convert_tail", "fwd_rebase_l"),
          ("ld_v_as_k_dq", "convert_stride", "fwd_rebase_qg"),
          ("ld_v_as_k_dkv", "convert_u0", "wide_dkv_row"),
          ("ld_do_as_o_dq", "split_last", "dq_mask"),
          ("ld_dv_as_dk", "ld_dv_as_dk_convert", "ws_clamp"),
          ("ld_do_as_q_dkv",),
          ("ld_o_as_q_delta",)]


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
    """one library per group of GROUPS: built side by side, the compiler runs outside the interpreter lock"""
    build_emu.build()                                   # the regular objects the mutant builds reuse
    assert sorted(name for group in GROUPS for name in group) == sorted(MUTANTS), "every mutant is in exactly one group"
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(8, len(os.sched_getaffinity(0))))) as pool:
        futs = {group: pool.submit(build_emu.build_mutant, str(tmp_path_factory.mktemp(group[0])), ATTN,
                                   [e for name in group for e in MUTANTS[name][0]]) for group in GROUPS}
        return {name: f.result() for group, f in futs.items() for name in group}


_passed_on_real_sources = set()


def _real_sources_pass(case):
    if case not in _passed_on_real_sources:             # several mutants share a case: the unmodified sources run it once
        with _use(build_emu.build()):
            CASES[case]()
        _passed_on_real_sources.add(case)


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_attention_mutant_is_caught(name, mutant_libs):
    _, fails, what, still_passes = MUTANTS[name]
    _real_sources_pass(fails)                           # the unmodified sources pass the very case ...
    with _use(mutant_libs[name]):
        with pytest.raises(AssertionError, match=what):
            CASES[fails]()                              # ... that the defect fails
        if still_passes is not None:
            CASES[still_passes]()                       # and the defect sits on the path only the killing case reaches
