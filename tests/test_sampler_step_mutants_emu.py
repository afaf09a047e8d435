"""The cases of tests/sampler_step_cases.py have teeth: the emulator library is rebuilt from a copy of the kernel sources with ONE
small defect in clora_sampler.hip each (tests/hipemu/build_emu.build_mutant, as tests/test_kernel_mutants_emu.py does for the other
kernels); the case named beside the defect must fail on the mutant and pass on the real sources, and where the defect sits on a
path only that case reaches, a second case must still pass on the mutant.

  halves_swapped   the guidance combine reads the cond half as uncond and the other way round
  hist_not_written this step's x0 never reaches `hist`
  x_in_cond_half   the second half of x_in (the conditional samples) is not written
  noise_dropped    the k_n * noise term is left out (inert for eta = 0)
  stride_h_for_n   the uncond half's sample offset uses es_h instead of es_n (inert for B = 1)
  grid_stride      the grid-stride loop strides twice its grid (inert until a thread takes a second trip: the launch past the cap)
  t_in_not_written the next timestep is not stored
  x_in_stale       x_in is rounded from the state before the update"""
import concurrent.futures
import contextlib
import os

import pytest

from controllora_amd import capi
from tests import sampler_step_cases as S
from tests.hipemu import build_emu

SRC = "clora_sampler.hip"

CASES = {
    "small_eta0": lambda: S.check_step((1, 4, 8, 8), "nchw", "ddim_eta0", "cpu"),
    "small_eta1": lambda: S.check_step((1, 4, 8, 8), "nhwc_padded", "ddim_eta1", "cpu"),
    "odd_dpm_second": lambda: S.check_step((3, 4, 5, 7), "nhwc_padded", "dpm_second", "cpu"),
    "odd_dense_dpm_second": lambda: S.check_step((3, 4, 5, 7), "nchw", "dpm_second", "cpu"),
    "past_cap": lambda: S.check_step(S.PAST_CAP, "nhwc_padded", "dpm_second", "cpu"),
    "apps_size": lambda: S.check_step((2, 4, 64, 64), "nhwc_padded", "dpm_second", "cpu"),
}

# mutant -> ([(old, new)], the case that must fail on it, what its assertion message must match or None, a case that must still pass or None)
MUTANTS = {
    "halves_swapped": ([("sampler_element(p.k, fu, fc, xv,", "sampler_element(p.k, fc, fu, xv,")], "small_eta0", r"x' ", None),
    "hist_not_written": ([("if (p.hist != nullptr) p.hist[at] = x0;", "if (false) p.hist[at] = x0;")], "small_eta0", r"hist ", None),
    "x_in_cond_half": ([("                p.x_in[at + cond] = r;\n", "")], "small_eta0", r"cond half", None),
    "noise_dropped": ([("if (use_n) acc += k.k_n * nz;", "if (false) acc += k.k_n * nz;")], "small_eta1", r"x' ", "small_eta0"),
    "stride_h_for_n": ([("p.eps + (long long)b * p.es_n", "p.eps + (long long)b * p.es_h")], "odd_dpm_second", None, "small_eta1"),
    "stride_h_for_n_dense": ([("p.eps + (long long)b * p.es_n", "p.eps + (long long)b * p.es_h")], "odd_dense_dpm_second", None, "small_eta0"),
    "grid_stride": ([("i < npix; i += (size_t)gridDim.x * 256)", "i < npix; i += (size_t)gridDim.x * 512)")], "past_cap", None, "apps_size"),
    "t_in_not_written": ([("threadIdx.x == 0) *p.t_in = p.t_next;", "threadIdx.x == 0) (void)p.t_next;")], "small_eta0", r"t_in", None),
    "x_in_stale": ([("const half_t r = (half_t)xn;", "const half_t r = (half_t)xv;")], "small_eta0", r"uncond half", None),
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
    """one library per distinct set of edits, built side by side (only clora_sampler.hip is recompiled)"""
    build_emu.build()                                   # the regular objects the mutant builds reuse
    builds = {}
    for name, (edits, *_rest) in MUTANTS.items():
        builds.setdefault(tuple(edits), name)
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(8, len(os.sched_getaffinity(0))))) as pool:
        futs = {key: pool.submit(build_emu.build_mutant, str(tmp_path_factory.mktemp(name)), SRC, list(key)) for key, name in builds.items()}
        libs = {key: f.result() for key, f in futs.items()}
    return {name: libs[tuple(edits)] for name, (edits, *_rest) in MUTANTS.items()}


_passed_on_real_sources = set()


def _real_sources_pass(case):
    if case not in _passed_on_real_sources:
        with _use(build_emu.build()):
            CASES[case]()
        _passed_on_real_sources.add(case)


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_sampler_mutant_is_caught(name, mutant_libs):
    _, fails, what, still_passes = MUTANTS[name]
    _real_sources_pass(fails)                           # the unmodified sources pass the very case ...
    with _use(mutant_libs[name]):
        with pytest.raises(AssertionError, match=what):
            CASES[fails]()                              # ... that the defect fails
        if still_passes is not None:
            CASES[still_passes]()                       # and the defect sits on the path only the killing case reaches
