"""GPU: the wide forward attention kernel (head dims 160 < D <= 512) on the real gfx950 library -- the cases of
tests/attention_wide_cases.py plus the two site shapes of the VAE's mid-block attention."""
import pytest
import torch

from tests import attention_wide_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("name", ["whole_tiles", "ragged_batch", "two_heads", "ragged_d"])
def test_wide_forward(name):
    W.case_plain(DEV, W.SHAPES[name])


def test_wide_forward_fused_168():
    W.case_fused_168(DEV)


def test_wide_forward_distinct_strides():
    W.case_strides(DEV)


def test_wide_forward_one_key():
    W.case_one_key(DEV)


def test_wide_forward_ramp():
    W.case_ramp(DEV)


def test_wide_forward_negative_first_tile():
    W.case_negative_first_tile(DEV)


@pytest.mark.parametrize("name", ["ragged_batch", "two_heads"])
def test_wide_forward_repeat_and_block_order(name):
    W.case_repeat_and_block_order(DEV, W.SHAPES[name])


def test_wide_forward_contract():
    W.case_contract(DEV)


@pytest.mark.parametrize("dims", [(1, 1, 9216, 9216, 512), (4, 1, 4096, 4096, 512)], ids=["decode_768", "encode_4x512"])
def test_wide_forward_site_shapes(dims):
    """the 768 x 768 decode (9,216 tokens: more than the materialised path can take) and the training encode"""
    W.case_plain(DEV, dims)
