"""The attention cases of tests/kernel_cases.py have teeth: the emulator library is rebuilt three times from a copy of the kernel
sources with ONE small defect each in clora_attn.hip (tests/hipemu/build_emu.build_mutant: only that translation unit is recompiled),
and the case that guards the mutated line must fail on the mutant and pass on the real sources.
  causal_mask   the causal mask hides the diagonal (`>=` for `>`): row 0 sees no key at all         -> case_attention_causal
  lse_units     the forward stores the LSE in base 2 (the conversion `* kLn2` dropped)              -> case_attention_full, LSE bound
  wide_dkv_row  the 8-wave dK/dV kernel -- and only it -- skips the last key row of a ragged block  -> case_attention_full under
                "attn_bwd_waves" 8, while the 4-wave kernels of the same library still pass"""
import contextlib

import pytest

from controllora_amd import capi
from tests import kernel_cases as KC
from tests.hipemu import build_emu

MUTANTS = {
    "causal_mask": [("if (kl >= rows || key > q0 + li) s[kt][0][r] = kNegBig;", "if (kl >= rows || key >= q0 + li) s[kt][0][r] = kNegBig;"),
                    ("if (kl >= rows || key > q0 + 16 + li) s[kt][1][r] = kNegBig;", "if (kl >= rows || key >= q0 + 16 + li) s[kt][1][r] = kNegBig;")],
    "lse_units": [("= (mref[qg] + log2f(lt)) * kLn2;", "= (mref[qg] + log2f(lt));")],
    "wide_dkv_row": [("        if (key < p.Nk) {\n", "        if (key < p.Nk && !(NWV == 8 && key == p.Nk - 1)) {\n")],
}


def _causal():
    KC.case_attention_causal("cpu", 2, 2, 77, 64)


def _full():
    KC.case_attention_full("cpu", 1, 2, 70, 150, 40)


def _wide(waves):
    def run():
        with KC.options(attn_bwd_waves=waves):
            KC.case_attention_full("cpu", 1, 2, 270, 130, 40, strided=True)
    return run


# mutant -> (the case that must fail on it, what its assertion names, a case that must still pass on the mutant library or None)
CASES = {"causal_mask": (_causal, None, None), "lse_units": (_full, r"\('lse', ", None), "wide_dkv_row": (_wide(8), r"\('dk', ", _wide(4))}


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
    return {name: build_emu.build_mutant(str(tmp_path_factory.mktemp(name)), "clora_attn.hip", edits) for name, edits in MUTANTS.items()}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_attention_mutant_is_caught(name, mutant_libs):
    fails, what, still_passes = CASES[name]
    with _use(mutant_libs[name]):
        with pytest.raises(AssertionError, match=what):
            fails()
        if still_passes is not None:
            still_passes()                              # the defect sits in the 8-wave kernel alone
    with _use(build_emu.build()):
        fails()                                         # and the unmodified sources pass the very same case
