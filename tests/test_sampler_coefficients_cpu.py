"""CPU: the coefficient form of the schedulers (schedulers `coefficients`: the eight numbers of the one-launch sampler step) against
their host `step`, both evaluated in fp64 on random tensors, for every step of the schedules the path uses; the extended DDIM step
with its defaults against the formula it had before it took `eta`; and the variance identity of eta = 1."""
import pytest
import torch

from controllora_amd.schedulers import COEF_NAMES, DDIMScheduler, DPMSolverMultistepScheduler

f64 = torch.float64
GUIDANCE = 7.5


def _tensors(seed, shape=(2, 4, 6, 5)):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*shape, generator=g, dtype=f64) for _ in range(4)]          # x, eps_u, eps_c, noise


def _linear_form(k, x, eu, ec, hist, noise):
    e = eu + k["guidance"] * (ec - eu)
    x0 = k["x0_x"] * x + k["x0_e"] * e
    return k["k_x"] * x + k["k_x0"] * x0 + k["k_h"] * hist + k["k_e"] * e + k["k_n"] * noise, x0


def _close(a, b, what):
    err = float((a - b).abs().max() / b.abs().max())
    assert err <= 1e-12, f"{what}: relative difference {err:.2e}"


@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("steps", [20, 50])
def test_ddim_coefficients_are_the_host_step(steps, eta):
    s = DDIMScheduler()
    s.set_timesteps(steps)
    x, eu, ec, noise = _tensors(steps)
    for i, t in enumerate(s.timesteps):
        k = s.coefficients(i, GUIDANCE, eta)
        assert tuple(k) == COEF_NAMES and all(isinstance(v, float) for v in k.values())
        got, _ = _linear_form(k, x, eu, ec, torch.zeros_like(x), noise)
        ref = s.step(eu + GUIDANCE * (ec - eu), t, x, eta=eta, noise=noise if eta else None)
        assert ref.dtype == f64
        _close(got, ref, f"DDIM-{steps} eta {eta} step {i}")
        assert (k["k_n"] == 0.0) == (eta == 0.0) and k["k_h"] == 0.0 and k["k_x"] == 0.0
        x = ref                                                   # walk the trajectory: realistic magnitudes at every step


@pytest.mark.parametrize("steps", [10, 20, 30])
def test_dpm_coefficients_are_the_host_step(steps):
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(steps)
    x, eu, ec, _ = _tensors(steps)
    hist, orders = torch.zeros_like(x), []
    for i, t in enumerate(s.timesteps):
        state = lambda: ([id(h) for h in s._x0_hist], list(s._t_hist), s._lower)
        before = state()
        k = s.coefficients(i, GUIDANCE)
        assert state() == before, "coefficients() touched the host history"
        assert tuple(k) == COEF_NAMES and k["k_e"] == 0.0 and k["k_n"] == 0.0
        got, x0 = _linear_form(k, x, eu, ec, hist, torch.zeros_like(x))
        ref = s.step(eu + GUIDANCE * (ec - eu), t, x)
        _close(got, ref, f"DPM-{steps} step {i}")
        _close(x0, s._x0_hist[-1], f"DPM-{steps} step {i} x0")
        orders.append(1 if k["k_h"] == 0.0 else 2)
        hist, x = x0, ref
        eu, ec = 0.9 * eu + 0.1 * ec, 0.9 * ec - 0.1 * eu          # another prediction per step
    want = [1] + [2] * (steps - 1)
    if steps < 15:
        want[-1] = 1                                                # lower_order_final
    assert orders == want


def test_ddim_step_defaults_are_the_former_formula_bit_for_bit():
    s = DDIMScheduler()
    for steps in (20, 50):
        s.set_timesteps(steps)
        for dtype in (torch.float32, torch.float16):
            g = torch.Generator().manual_seed(steps)
            sample, eps = torch.randn(2, 4, 8, 8, generator=g).to(dtype), torch.randn(2, 4, 8, 8, generator=g).to(dtype)
            for t in s.timesteps:
                prev = t - s.num_train_timesteps // s.num_inference_steps
                a_t = float(s.alphas_cumprod[t])
                a_p = float(s.alphas_cumprod[prev] if prev >= 0 else s.alphas_cumprod[0])
                x0 = (sample.float() - (1 - a_t) ** 0.5 * eps.float()) / a_t ** 0.5
                former = (a_p ** 0.5 * x0 + (1 - a_p) ** 0.5 * eps.float()).to(sample.dtype)
                assert torch.equal(s.step(eps, t, sample), former)
                assert torch.equal(s.step(eps, t, sample, eta=0.0, noise=None), former)


def test_eta_one_is_the_ddpm_variance_split():
    for steps in (20, 50):
        s = DDIMScheduler()
        s.set_timesteps(steps)
        for i, t in enumerate(s.timesteps):
            k = s.coefficients(i, GUIDANCE, 1.0)
            _, a_p = s._alphas(t)
            assert abs(k["k_e"] ** 2 + k["k_n"] ** 2 - (1 - a_p)) <= 1e-12, (steps, i)


def test_coefficient_order_is_the_struct_of_the_header():
    import os
    import re
    from controllora_amd import capi, kernels as K
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    decl = re.search(r"typedef struct \{ float ([a-z0-9_, ]+); \} clora_sampler_coef_t;", open(os.path.join(root, "include", "clora.h")).read())
    assert tuple(n.strip() for n in decl.group(1).split(",")) == COEF_NAMES == K.SAMPLER_COEF_NAMES
    assert [n for n, _ in capi.SamplerCoef._fields_] == list(COEF_NAMES)


def test_eta_needs_noise_and_dpm_has_no_eta():
    s = DDIMScheduler()
    s.set_timesteps(20)
    x = torch.zeros(1, 4, 2, 2)
    with pytest.raises(ValueError, match="noise"):
        s.step(x, s.timesteps[0], x, eta=0.5)
    with pytest.raises(TypeError):
        DPMSolverMultistepScheduler().coefficients(0, GUIDANCE, 0.5)
