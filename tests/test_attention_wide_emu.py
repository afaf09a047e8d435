"""CPU (host-emulated kernels, tiny shapes): the wide forward attention kernel (head dims 160 < D <= 512), its contract, the narrow
kernels' unchanged bits, and -- in the style of tests/test_attention_mutants_emu.py -- four mutants of clora_attn_wide.hip: the ragged
key mask, and the table WIDE_MUTANTS below (a V tile fetched with K's row stride, the odd-k-step partial sum, the rebase of the
running sum)."""
import contextlib

import pytest
import torch

from controllora_amd import capi
from tests import attention_wide_cases as W
from tests.emu_fixture import use_emulator
from tests.hipemu import build_emu


@pytest.fixture(autouse=True)
def _emulated():
    with use_emulator():
        yield


@pytest.mark.parametrize("name", ["whole_tiles", "ragged_batch", "two_heads", "ragged_d"])
def test_wide_forward(name):
    W.case_plain("cpu", W.SHAPES[name])


def test_wide_forward_fused_168():
    W.case_fused_168("cpu")


def test_wide_forward_one_key():
    W.case_one_key("cpu")


def test_wide_forward_ramp():
    W.case_ramp("cpu")


def test_wide_forward_negative_first_tile():
    W.case_negative_first_tile("cpu")


@pytest.mark.parametrize("name", ["ragged_batch", "two_heads"])
def test_wide_forward_repeat_and_block_order(name):
    W.case_repeat_and_block_order("cpu", W.SHAPES[name])


def test_wide_forward_contract():
    W.case_contract("cpu")


def test_narrow_forward_bits_did_not_move():
    """D = 40 still runs the kernels of clora_attn.hip: o and lse equal the bits the emulator build of the commit before the wide
    kernel produced (tests/golden/attn_narrow_fwd_emu.pt, recorded from that build with the inputs of narrow_forward)"""
    want = torch.load(W.NARROW_GOLDEN)
    o, lse = W.narrow_forward("cpu")
    assert torch.equal(o, want["o"]) and torch.equal(lse, want["lse"])


def test_wide_mutant_without_the_ragged_key_mask_is_caught(tmp_path):
    """the keys a ragged last tile does not have are zero rows in LDS: unmasked they would each weigh exp(0 - max) in the softmax"""
    build_emu.build()                                   # the regular objects the mutant build reuses
    lib = build_emu.build_mutant(str(tmp_path), "clora_attn_wide.hip",
                                 [("if (kt * 16 + 4 * g + r >= rows) {", "if (false && kt * 16 + 4 * g + r >= rows) {")])
    old = capi._LIB
    capi._LIB = capi.Lib(lib, require_device=False)
    try:
        with pytest.raises(AssertionError, match=r"\('o', "):
            W.case_plain("cpu", W.SHAPES["ragged_batch"])
        W.case_plain("cpu", W.SHAPES["whole_tiles"])    # no ragged tile: the mutant is right
    finally:
        capi._LIB = old
    W.case_plain("cpu", W.SHAPES["ragged_batch"])       # and the real sources pass the very same case


def test_wide_forward_distinct_strides():
    W.case_strides("cpu")


WIDE_CASES = {"strides": lambda: W.case_strides("cpu"), "ramp": lambda: W.case_ramp("cpu"),
              "whole_tiles": lambda: W.case_plain("cpu", W.SHAPES["whole_tiles"]), "two_heads": lambda: W.case_plain("cpu", W.SHAPES["two_heads"]),
              "ragged_batch": lambda: W.case_plain("cpu", W.SHAPES["ragged_batch"])}
_V_NEXT = "dma.template issue<false>(vbase + (size_t)(kv0 + BKV) * p.ldv, p.ldv, nrows, nb + BKV * LD, w);"
# mutant -> ([(old, new)] of clora_attn_wide.hip, the case that must fail with ('o', ...), a case that still passes on the mutant library)
#   wide_ld_v_as_k  the V tiles after the first are fetched with K's row stride: survived every case until case_strides (k and v always
#                   had one stride)
#   wide_s2         the last odd k-step's partial sum multiplies the Q fragment two steps back: channels 480..511, so D = 256 passes
#   wide_rebase_l   a rebase after the first tile does not rescale the running sum
WIDE_MUTANTS = {
    "wide_ld_v_as_k": ([(_V_NEXT, _V_NEXT.replace("p.ldv, nrows", "p.ldk, nrows"))], "strides", "two_heads"),
    "wide_s2": ([("if (SP == 2 && (ks & 1)) s2[kt][qg] = mfma16(a, qf[qg][ks], s2[kt][qg]);",
                  "if (SP == 2 && (ks & 1)) s2[kt][qg] = mfma16(a, qf[qg][ks == KS - 1 ? ks - 2 : ks], s2[kt][qg]);")], "whole_tiles", "two_heads"),
    "wide_rebase_l": ([("lrun[qg] *= alpha;", "lrun[qg] *= 1.f;")], "ramp", "ragged_batch"),
}
WIDE_GROUPS = [("wide_ld_v_as_k", "wide_s2"), ("wide_rebase_l",)]    # one compilation each: the first two meet in no case named above


@pytest.fixture(scope="module")
def wide_mutant_libs(tmp_path_factory):
    import concurrent.futures
    build_emu.build()
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(WIDE_GROUPS)) as pool:
        futs = {group: pool.submit(build_emu.build_mutant, str(tmp_path_factory.mktemp(group[0])), "clora_attn_wide.hip",
                                   [e for name in group for e in WIDE_MUTANTS[name][0]]) for group in WIDE_GROUPS}
        return {name: f.result() for group, f in futs.items() for name in group}


@pytest.mark.parametrize("name", sorted(WIDE_MUTANTS))
def test_wide_mutant_is_caught(name, wide_mutant_libs):
    _, fails, still_passes = WIDE_MUTANTS[name]
    WIDE_CASES[fails]()                                 # the real sources pass the very case ...
    old = capi._LIB
    capi._LIB = capi.Lib(wide_mutant_libs[name], require_device=False)
    try:
        with pytest.raises(AssertionError, match=r"\('o', "):
            WIDE_CASES[fails]()                         # ... that the defect fails, naming the output
        WIDE_CASES[still_passes]()                      # and the defect sits on the path only the killing case reaches
    finally:
        capi._LIB = old
