"""The cases of tests/openpose_cases.py have teeth: the emulator library is rebuilt from a copy of the kernel sources with ONE small
defect in clora_pose.hip each (tests/hipemu/build_emu.build_mutant, as tests/test_kernel_mutants_emu.py does for the other kernels);
the case named beside the defect must fail on the mutant and pass on the real sources.

  halo_short        the first row of the staged input patch is left zero (the halo one pixel short at the top)
  relu_dropped      the activation is the identity
  bias_in_slabs     every split-K slab already carries the bias, the finish pass adds it once more
  job1_reads_w0     the second job reads the first job's weights
  cout_rounded_up   the store covers Cout rounded up to 8 channels"""
import concurrent.futures
import contextlib
import os

import pytest

from controllora_amd import capi
from tests import openpose_cases as C
from tests.hipemu import build_emu

SRC = "clora_pose.hip"

CASES = {
    "conv7_ragged": lambda: C.case_conv_act("cpu", *C.CONV7[1], 7, relus=(False,)),
    "conv3_relu": lambda: C.case_conv_act("cpu", *C.CONV3[1], 3, relus=(True,)),
    "conv7_small_split": lambda: C.case_conv_act("cpu", *C.CONV7[0], 7, relus=(False,)),
    "conv1_two_jobs": lambda: C.case_conv_act("cpu", *C.CONV1[0], 1, relus=(False, False)),
    "heads": lambda: C.case_heads("cpu", 1, 5, 7),
}

# mutant -> ([(old, new)], the case that must fail on it)
MUTANTS = {
    "halo_short": ([("if (y >= 0 && y < P.H && x >= 0 && x < P.W && ci < J.Cin) v =", "if (py >= 1 && y >= 0 && y < P.H && x >= 0 && x < P.W && ci < J.Cin) v =")],
                   "conv7_ragged"),
    "relu_dropped": ([("{ return relu ? fmaxf(v, 0.f) : v; }", "{ return v; }")], "conv3_relu"),
    "bias_in_slabs": ([("const float part = acc[f][r];", "const float part = acc[f][r] + bias_v;")], "conv7_small_split"),
    "job1_reads_w0": ([("const half_t* wl = J.w + ", "const half_t* wl = P.job[0].w + ")], "conv1_two_jobs"),
    "cout_rounded_up": ([("void store_pair(half_t* yrow, int co, int Cout, float v0, float v1) {",
                          "void store_pair(half_t* yrow, int co, int Cout, float v0, float v1) {\n    Cout = (Cout + 7) & ~7;")], "heads"),
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
    build_emu.build()                                   # the regular objects the mutant builds reuse
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(8, len(os.sched_getaffinity(0))))) as pool:
        futs = {name: pool.submit(build_emu.build_mutant, str(tmp_path_factory.mktemp(name)), SRC, list(edits)) for name, (edits, _) in MUTANTS.items()}
        return {name: f.result() for name, f in futs.items()}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_pose_mutant_is_caught(name, mutant_libs):
    _, fails = MUTANTS[name]
    with _use(build_emu.build()):
        CASES[fails]()                                  # the unmodified sources pass the very case ...
    with _use(mutant_libs[name]):
        with pytest.raises(AssertionError):
            CASES[fails]()                              # ... that the defect fails
