"""CPU (host-emulated kernels, tiny shapes): the wide forward attention kernel (head dims 160 < D <= 512), its contract, the narrow
kernels' unchanged bits, and -- in the style of tests/test_attention_mutants_emu.py -- one mutant of clora_attn_wide.hip that the
ragged case must catch."""
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
