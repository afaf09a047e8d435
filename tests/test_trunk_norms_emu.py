"""CPU tests: the norms that read the compensated trunk (CLORA_TRUNK_LO=norms) on the host-emulated kernels -- the shapes
tests/test_kernels_emu.py uses for the same plans (tests/trunk_norm_cases.py states the limits)."""
import pytest

from tests import trunk_norm_cases as TC
from tests.emu_fixture import use_emulator


@pytest.fixture(autouse=True)
def _emu():
    with use_emulator():
        yield


# two launches, one block per slab, team (HW >= 1024), the ragged two-launch shape with SiLU
@pytest.mark.parametrize("B,HW,C,G", [(2, 256, 320, 32), (2, 64, 1280, 32), (1, 1024, 320, 32), (2, 300, 64, 8)])
def test_groupnorm_reads_hi_plus_lo(B, HW, C, G):
    TC.case_groupnorm_lo("cpu", B, HW, C, G)


def test_groupnorm_reads_hi_plus_lo_with_silu():
    TC.case_groupnorm_lo("cpu", 2, 300, 64, 8, silu=True)


@pytest.mark.parametrize("B,HW,Ca,Cb,G,silu", [(1, 256, 640, 320, 32, True), (1, 300, 64, 32, 8, False), (2, 9, 1280, 640, 32, True),
                                               (1, 1024, 320, 640, 32, False), (3, 37, 8, 56, 8, True)])
def test_groupnorm_concat_reads_hi_plus_lo(B, HW, Ca, Cb, G, silu):
    TC.case_groupnorm_lo_concat("cpu", B, HW, Ca, Cb, G, silu)


def test_groupnorm_lo_rejects_a_deferred_source():
    TC.case_groupnorm_lo_rejects_deferred("cpu")


@pytest.mark.parametrize("M,C", [(37, 320), (9, 1280), (5, 64), (2051, 320), (2050, 640), (2049, 1280), (309, 320), (77, 1280), (130, 768)])
def test_layernorm_reads_hi_plus_lo(M, C):
    TC.case_layernorm_lo("cpu", M, C)


def test_blocks_in_norms_mode():
    TC.case_blocks_norms("cpu")


def test_small_unet_modes(monkeypatch):
    unet, _, inp, _ = TC.case_small_unet_modes("cpu", monkeypatch)
    TC.check_infer_is_trunklo_true(unet, inp, "cpu", monkeypatch)
