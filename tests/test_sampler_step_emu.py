"""CPU tests of the one-launch sampler step on the emulated kernels: the kernel against the fp64 form at every shape, layout and
coefficient set of tests/sampler_step_cases.py, its properties and argument errors, and pipeline.ddim_sample(step_impl="device")
with a stub eps model, teacher-forced step by step against the fp64 host schedulers."""
import pytest
import torch

from tests import sampler_step_cases as S
from tests.emu_fixture import use_emulator


@pytest.fixture(autouse=True)
def _emu():
    with use_emulator():
        yield


@pytest.mark.parametrize("name", S.COEF_SETS)
@pytest.mark.parametrize("layout", S.LAYOUTS)
@pytest.mark.parametrize("shape", [s for s in S.SHAPES if s != S.PAST_CAP])
def test_step_against_fp64(shape, layout, name):
    S.check_step(shape, layout, name, "cpu")


@pytest.mark.parametrize("name", S.PAST_CAP_SETS)
@pytest.mark.parametrize("layout", S.LAYOUTS)
def test_step_past_the_grid_cap_against_fp64(layout, name):
    S.check_step(S.PAST_CAP, layout, name, "cpu")


@pytest.mark.parametrize("layout", S.LAYOUTS)
@pytest.mark.parametrize("shape", [(3, 4, 5, 7), (2, 4, 64, 64)])
def test_step_properties(shape, layout):
    S.check_properties(shape, layout, "cpu")


def test_step_argument_errors():
    S.check_argument_errors("cpu")


def _loop_inputs(B=2, H=8, W=8):
    g = torch.Generator().manual_seed(3)
    return dict(cond=torch.zeros(B, 77, 8).half(), uncond=torch.zeros(B, 77, 8).half(), latents=torch.randn(B, 4, H, W, generator=g).half())


@pytest.mark.parametrize("name", sorted(S.LOOPS))
def test_device_loop_teacher_forced(name):
    S.check_teacher_forced(name, S.StubUNet(), None, None, **_loop_inputs())


def test_device_loop_eta_zero_is_the_loop_without_eta():
    a, _ = S.run_loop("ddim8", S.StubUNet(), None, None, **_loop_inputs())
    b, _ = S.run_loop("ddim8", S.StubUNet(), None, None, eta=0.0, **_loop_inputs())
    assert torch.equal(a, b)
    c, _ = S.run_loop("dpm8", S.StubUNet(), None, None, **_loop_inputs())
    d, _ = S.run_loop("dpm8", S.StubUNet(), None, None, eta=0.7, **_loop_inputs())        # DPM-Solver++ ignores eta
    assert torch.equal(c, d)


@pytest.mark.parametrize("name", sorted(S.LOOPS))
def test_device_loop_against_host_loop(name):
    """the two step implementations on the same model and noise: reported, and loosely bounded here because the stub model is
    smooth (fp32 summation order only; through a real fp16 UNet the difference is amplified and is not asserted anywhere)"""
    dev, _ = S.run_loop(name, S.StubUNet(), None, None, **_loop_inputs())
    host, _ = S.run_loop(name, S.StubUNet(), None, None, step_impl="host", **_loop_inputs())
    err = float((dev - host).norm() / host.norm())
    print(f"SAMPLER_LOOP {name}: device against host final latents rel-L2 {err:.3e}")
    assert torch.isfinite(dev).all() and err < 1e-2


def test_generator_noise_is_drawn_once_per_step_on_both_paths():
    """eta > 0 without a noise tensor: both paths draw one randn per step from the generator, in the same order"""
    outs = []
    for impl in ("host", "device"):
        g = torch.Generator().manual_seed(11)
        out, _ = S.run_loop("ddim8", S.StubUNet(), None, None, step_impl=impl, eta=1.0, generator=g, **_loop_inputs())
        outs.append((out, g.get_state().clone()))
    assert torch.equal(outs[0][1], outs[1][1]), "the two paths consumed the generator differently"
    assert float((outs[0][0] - outs[1][0]).norm() / outs[0][0].norm()) < 1e-2
    plain, _ = S.run_loop("ddim8", S.StubUNet(), None, None, **_loop_inputs())
    assert float((outs[1][0] - plain).abs().max()) > 1e-2, "eta = 1 changed nothing"


def test_unknown_step_impl_and_bad_noise_shape():
    with pytest.raises(ValueError, match="step_impl"):
        S.run_loop("ddim8", S.StubUNet(), None, None, step_impl="gpu", **_loop_inputs())
    from controllora_amd.pipeline import ddim_sample
    inp = _loop_inputs()
    with pytest.raises(ValueError, match="noise"):
        ddim_sample(S.StubUNet(), None, None, inp["cond"], inp["uncond"], steps=8, latents=inp["latents"], eta=0.5,
                    noise=torch.zeros(7, 2, 4, 8, 8), graph=False, step_impl="device")
