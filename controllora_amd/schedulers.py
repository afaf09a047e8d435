"""Noise schedules used on the path: DDPM ``add_noise`` for training
(reference train_text_to_image_control_lora.py:399, 765), the DDIM update of the BASELINE inference configuration (eta = 0; any
eta on request) and DPM-Solver++(2M).  `step` is scalar / per-sample coefficient math in tiny torch ops; `coefficients` gives the
same update as the eight numbers of the one-launch sampler step (include/clora.h clora_sampler_step_f16)."""
from __future__ import annotations

import math

import torch

# the linear form every sampler of the path is an instance of (kernels.sampler_step):
#   e = eps_u + guidance * (eps_c - eps_u);  x0 = x0_x x + x0_e e;  x' = k_x x + k_x0 x0 + k_h hist + k_e e + k_n noise
COEF_NAMES = ("guidance", "x0_x", "x0_e", "k_x", "k_x0", "k_h", "k_e", "k_n")


def _wide(t):
    """the fp32 the updates are formed in; an fp64 tensor stays fp64 (tests evaluate a step in fp64)"""
    return t if t.dtype == torch.float64 else t.float()


class DDPMScheduler:
    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, prediction_type="epsilon"):
        self.num_train_timesteps = num_train_timesteps
        self.prediction_type = prediction_type
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.init_noise_sigma = 1.0

    def add_noise(self, original_samples, noise, timesteps):
        ac = self.alphas_cumprod.to(device=original_samples.device, dtype=original_samples.dtype)
        a = ac[timesteps].sqrt().reshape(-1, 1, 1, 1)
        s = (1 - ac[timesteps]).sqrt().reshape(-1, 1, 1, 1)
        return a * original_samples + s * noise


    def get_velocity(self, sample, noise, timesteps):
        """v-prediction target (reference train...:776-777): sqrt(a_t) * noise - sqrt(1 - a_t) * sample"""
        ac = self.alphas_cumprod.to(device=sample.device, dtype=sample.dtype)
        a = ac[timesteps].sqrt().reshape(-1, 1, 1, 1)
        s = (1 - ac[timesteps]).sqrt().reshape(-1, 1, 1, 1)
        return a * noise - s * sample


class DDIMScheduler(DDPMScheduler):
    """steps_offset = 1, set_alpha_to_one = False (the SD-1.5 scheduler config); eta = 0 unless a step asks for more."""

    def set_timesteps(self, n):
        self.num_inference_steps = n
        ratio = self.num_train_timesteps // n
        self.timesteps = [int(i * ratio) + 1 for i in reversed(range(n))]

    def _alphas(self, t):
        prev = t - self.num_train_timesteps // self.num_inference_steps
        return float(self.alphas_cumprod[t]), float(self.alphas_cumprod[prev] if prev >= 0 else self.alphas_cumprod[0])

    @staticmethod
    def _sigma(a_t, a_p, eta):
        return eta * ((1 - a_p) / (1 - a_t)) ** 0.5 * (1 - a_t / a_p) ** 0.5

    def step(self, eps, t, sample, eta=0.0, noise=None):
        """eta > 0 (DDIM's stochastic family, eta = 1: the DDPM variance) needs `noise`, standard normal like `sample`"""
        a_t, a_p = self._alphas(t)
        x0 = (_wide(sample) - (1 - a_t) ** 0.5 * _wide(eps)) / a_t ** 0.5
        if not eta:
            return (a_p ** 0.5 * x0 + (1 - a_p) ** 0.5 * _wide(eps)).to(sample.dtype)
        if noise is None:
            raise ValueError("a DDIM step with eta > 0 needs its noise")
        sigma = self._sigma(a_t, a_p, float(eta))
        return (a_p ** 0.5 * x0 + (1 - a_p - sigma ** 2) ** 0.5 * _wide(eps) + sigma * _wide(noise)).to(sample.dtype)

    def coefficients(self, i, guidance_scale, eta=0.0):
        """step i (0-based index into `timesteps`) as the eight numbers of COEF_NAMES, in Python floats"""
        a_t, a_p = self._alphas(self.timesteps[i])
        sigma = self._sigma(a_t, a_p, float(eta))
        return dict(guidance=float(guidance_scale), x0_x=1.0 / a_t ** 0.5, x0_e=-((1 - a_t) ** 0.5) / a_t ** 0.5, k_x=0.0,
                    k_x0=a_p ** 0.5, k_h=0.0, k_e=(1 - a_p - sigma ** 2) ** 0.5, k_n=sigma)


class DPMSolverMultistepScheduler(DDPMScheduler):
    """DPM-Solver++(2M), epsilon prediction, `lower_order_final` -- the sampler the reference apps switch to
    (apps/gradio_canny2image.py:34, train...:817: `DPMSolverMultistepScheduler.from_config(...)`, upstream defaults:
    algorithm_type "dpmsolver++", solver_order 2, solver_type "midpoint").  Restated from the DPM-Solver++ paper
    (Lu et al. 2022, eqs. for the data-prediction multistep solver); upstream diffusers is absent, so this is PARITY
    UNPINNED against it -- tests pin the identities that must hold (first order == DDIM(eta=0); an exact-x0 model is
    integrated exactly by both orders).  Scalar coefficient math on the host; the latents stay on the device."""

    def __init__(self, *a, solver_order=2, lower_order_final=True, **kw):
        super().__init__(*a, **kw)
        self.solver_order, self.lower_order_final = solver_order, lower_order_final
        acp = self.alphas_cumprod.double()
        self._alpha, self._sigma = acp.sqrt(), (1 - acp).sqrt()
        self._lambda = torch.log(self._alpha) - torch.log(self._sigma)

    def set_timesteps(self, n):
        self.num_inference_steps = n
        ts = torch.linspace(0, self.num_train_timesteps - 1, n + 1).round().long().flip(0)[:-1]
        self.timesteps = [int(t) for t in ts]
        self._x0_hist, self._t_hist, self._lower = [], [], 0

    def _coef(self, t):
        if t < 0:                      # "final" step integrates to clean data: alpha = 1, sigma = 0
            return 1.0, 0.0, float("inf")
        return float(self._alpha[t]), float(self._sigma[t]), float(self._lambda[t])

    def _first_order(self, i):
        """the order logic of `step` as a function of the step index: the first step has no history; with `lower_order_final` the last
        step of a short schedule (fewer than 15 steps) falls back to first order"""
        last = i == len(self.timesteps) - 1
        return self.solver_order == 1 or i == 0 or (self.lower_order_final and last and len(self.timesteps) < 15)

    def coefficients(self, i, guidance_scale):
        """step i (0-based index into `timesteps`) as the eight numbers of COEF_NAMES, in Python floats; `hist` of the form is the
        previous step's x0.  Reads the schedule only: the host history of `step` is neither used nor changed."""
        t = self.timesteps[i]
        prev = self.timesteps[i + 1] if i + 1 < len(self.timesteps) else 0
        a_s, s_s, l_s = self._coef(t)
        a_t, s_t, l_t = self._coef(prev)
        h = l_t - l_s
        k_x0, k_h = -a_t * math.expm1(-h), 0.0
        if not self._first_order(i):
            r0 = (l_s - float(self._lambda[self.timesteps[i - 1]])) / h
            k_x0, k_h = k_x0 * (1.0 + 0.5 / r0), -0.5 * k_x0 / r0
        return dict(guidance=float(guidance_scale), x0_x=1.0 / a_s, x0_e=-s_s / a_s, k_x=s_t / s_s, k_x0=k_x0, k_h=k_h, k_e=0.0, k_n=0.0)

    def step(self, eps, t, sample):
        i = self.timesteps.index(int(t))
        prev = self.timesteps[i + 1] if i + 1 < len(self.timesteps) else 0
        a_s, s_s, l_s = self._coef(int(t))
        a_t, s_t, l_t = self._coef(prev)
        x = _wide(sample)
        x0 = (x - s_s * _wide(eps)) / a_s
        self._x0_hist = (self._x0_hist + [x0])[-self.solver_order:]
        self._t_hist = (self._t_hist + [int(t)])[-self.solver_order:]
        h = l_t - l_s
        em1 = math.expm1(-h)                                       # e^{-h} - 1
        last = i == len(self.timesteps) - 1
        first_order = self.solver_order == 1 or self._lower < 1 or (self.lower_order_final and last and len(self.timesteps) < 15)
        if first_order:
            out = (s_t / s_s) * x - a_t * em1 * x0
        else:
            m0, m1 = self._x0_hist[-1], self._x0_hist[-2]
            l_s1 = float(self._lambda[self._t_hist[-2]])
            r0 = (l_s - l_s1) / h
            d1 = (m0 - m1) / r0
            out = (s_t / s_s) * x - a_t * em1 * m0 - 0.5 * a_t * em1 * d1
        if self._lower < self.solver_order:
            self._lower += 1
        return out.to(sample.dtype)
