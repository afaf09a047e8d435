"""GPU twins (-m gpu) of tests/test_gemm_tiles_emu.py: the GEMM tile table of the gfx950 library (tests/tile_table_cases.py)."""
import pytest

from tests import kernel_cases as KC
from tests import tile_table_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True, scope="module")
def _native_lib_loaded():
    from controllora_amd import capi
    L = capi.lib()
    assert L.require_device and L.path.endswith("libclora.so")
    yield


def test_rows_are_the_pinned_table():
    TC.case_rows_are_the_pinned_table()


def test_plain_launch_accepts_exactly_the_rows():
    TC.case_plain_launch_accepts_exactly_the_rows(DEV)


def test_fused_down_rule():
    TC.case_fused_down_rule()


@pytest.mark.parametrize("tile", TC.D_ROWS)
def test_d_rows_carry_the_down_projection(tile):
    TC.case_d_row(DEV, tile)


def test_ln_bits():
    TC.case_ln_bits(DEV)


@pytest.mark.parametrize("tile", TC.L_ROWS)
def test_l_rows_fuse_the_layernorm(tile):
    KC.case_gemm_fused_layernorm(DEV, 150, 64, tile)


@pytest.mark.parametrize("tile", TC.G_ROWS)
def test_g_rows_run_the_geglu_forward(tile):
    KC.case_feed_forward_fused(DEV, M=150, C=64, tile_cfg=tile)


@pytest.mark.parametrize("tile", TC.PATCH_ROWS)
def test_patch_rows(tile):
    TC.case_patch_row(DEV, tile)
