"""CPU tests of the GEMM tile table (tests/tile_table_cases.py) on the host emulator build of the library."""
import pytest

from tests import kernel_cases as KC
from tests import tile_table_cases as TC
from tests.emu_fixture import use_emulator


@pytest.fixture(autouse=True)
def _emu():
    with use_emulator():
        yield


def test_rows_are_the_pinned_table():
    TC.case_rows_are_the_pinned_table()


def test_plain_launch_accepts_exactly_the_rows():
    TC.case_plain_launch_accepts_exactly_the_rows("cpu")


def test_fused_down_rule():
    TC.case_fused_down_rule()


@pytest.mark.parametrize("tile", TC.D_ROWS)
def test_d_rows_carry_the_down_projection(tile):
    TC.case_d_row("cpu", tile)


def test_ln_bits():
    TC.case_ln_bits("cpu")


@pytest.mark.parametrize("tile", TC.L_ROWS)
def test_l_rows_fuse_the_layernorm(tile):
    KC.case_gemm_fused_layernorm("cpu", 150, 64, tile)


@pytest.mark.parametrize("tile", TC.G_ROWS)
def test_g_rows_run_the_geglu_forward(tile):
    KC.case_feed_forward_fused("cpu", M=150, C=64, tile_cfg=tile)


@pytest.mark.parametrize("tile", TC.PATCH_ROWS)
def test_patch_rows(tile):
    TC.case_patch_row("cpu", tile)
