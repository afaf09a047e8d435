"""Shared cases of the one-launch sampler step (clora_sampler_step_f16, kernels.sampler_step) and of the sampling loop that uses it
(pipeline.ddim_sample(step_impl="device")): run on the emulated kernels by tests/test_sampler_step_emu.py and on the real library by
tests/test_sampler_step_gpu.py.

The kernel is checked against an fp64 restatement of its three lines

    e  = eps_u + guidance * (eps_c - eps_u)
    x0 = x0_x * x + x0_e * e
    x' = k_x * x + k_x0 * x0 + k_h * hist + k_e * e + k_n * noise

elementwise: |out - ref| <= ROUNDINGS * 2^-24 * S, S the same expression with every term replaced by its absolute value
(S = |k_x x| + |k_x0| (|x0_x x| + |x0_e| E) + |k_h hist| + |k_e| E + |k_n noise|, E = |eps_u| + |guidance| (|eps_c| + |eps_u|); for
`hist`, which receives x0: S = |x0_x x| + |x0_e| E).  ROUNDINGS = 12 counts the fp32 roundings on the longest path from an input to
x': two coefficient roundings (the fp64 coefficient to fp32, on the two factors a term passes: x0_e and k_x0), three in e (the
difference, the product, the sum), three in x0 (two products, one sum), and the four products and sums of the outer line that the
x0 term passes.  Each rounding is at most 2^-24 relative to a partial result that S bounds.  No measured slack is added: a numpy fp32
evaluation of the same lines stays below 4 * 2^-24 * S over every step of DDIM 20 / 50 at eta 0, 0.5, 1 and DPM-Solver++ 10 / 20 / 30."""
import functools

import torch

from controllora_amd import capi, kernels as K
from controllora_amd.schedulers import COEF_NAMES, DDIMScheduler, DPMSolverMultistepScheduler

f16, f32, f64 = torch.float16, torch.float32, torch.float64
U = 2.0 ** -24
ROUNDINGS = 12
MAX_BLOCKS = 1024            # SAMPLER_MAX_BLOCKS of clora_sampler.hip: the grid is capped at this many blocks of 256 one-pixel threads
# (B, C, H, W): one block; nothing divisible by a vector width; the apps' 512 x 512 latent at two images; C != 4 (the path without the
# one-load-per-pixel form, whatever the layout); and the smallest launch in which a thread takes a second trip of the capped
# grid-stride loop: B * H * W = MAX_BLOCKS * 256 + 1 pixels (thread 0 of block 0 owns the last one)
PAST_CAP = (1, 4, 5, 52429)
assert PAST_CAP[0] * PAST_CAP[2] * PAST_CAP[3] == MAX_BLOCKS * 256 + 1
SHAPES = [(1, 4, 8, 8), (3, 4, 5, 7), (2, 4, 64, 64), (2, 3, 6, 5), PAST_CAP]
LAYOUTS = ["nchw", "nhwc_padded"]


@functools.lru_cache(maxsize=None)
def coef_sets():
    """real coefficient sets of the schedulers: a DDIM step at eta 0 and 1, a DPM-Solver++ step of first and of second order, and the
    last step of each (the 20-step DPM schedule ends in a second-order step, the 8-step one in `lower_order_final`'s first-order)"""
    ddim, dpm, dpm8 = DDIMScheduler(), DPMSolverMultistepScheduler(), DPMSolverMultistepScheduler()
    ddim.set_timesteps(20); dpm.set_timesteps(20); dpm8.set_timesteps(8)
    sets = {"ddim_eta0": ddim.coefficients(7, 7.5), "ddim_eta1": ddim.coefficients(7, 7.5, 1.0),
            "ddim_eta0_last": ddim.coefficients(19, 9.0), "ddim_eta1_last": ddim.coefficients(19, 9.0, 1.0),
            "dpm_first": dpm.coefficients(0, 7.5), "dpm_second": dpm.coefficients(7, 7.5),
            "dpm_second_last": dpm.coefficients(19, 7.5), "dpm_first_last": dpm8.coefficients(7, 7.5)}
    assert sets["ddim_eta0"]["k_n"] == 0 and sets["ddim_eta1"]["k_n"] > 0 and sets["ddim_eta1_last"]["k_n"] > 0
    assert sets["dpm_first"]["k_h"] == 0 and sets["dpm_first_last"]["k_h"] == 0
    assert sets["dpm_second"]["k_h"] != 0 and sets["dpm_second_last"]["k_h"] != 0
    return sets


COEF_SETS = sorted(coef_sets())
# the launch past the cap differs from the others in its trip count alone, which no coefficient changes: it runs the two sets that
# between them have every term of the form (noise and k_e; hist and k_x)
PAST_CAP_SETS = ["ddim_eta1", "dpm_second"]


def make_eps(shape, layout, dev, seed=0, offset=0):
    """fp16 noise prediction [2B,C,H,W] as a dense NCHW tensor, or as the NHWC view of a padded buffer -- rows of 8 channels of which
    the first C are valid, 3 pixels of padding per row, one row of padding per sample: the four strides are pairwise distinct and none
    is the dense one.  The padding is NaN: a kernel that reads it shows.  `offset` shifts the view by that many elements."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(1000 * seed + 131 * B + 17 * H + W)
    val = torch.randn(2 * B, C, H, W, generator=g).half()
    if layout == "nchw":
        return val.to(dev)
    CP = 8
    buf = torch.full((2 * B * (H + 1) * (W + 3) * CP + 8,), float("nan"), dtype=f16)
    view = buf[offset:offset + 2 * B * (H + 1) * (W + 3) * CP].view(2 * B, H + 1, W + 3, CP)[:, :H, :W, :C].permute(0, 3, 1, 2)
    view.copy_(val)
    buf = buf.to(dev)
    view = buf[offset:offset + 2 * B * (H + 1) * (W + 3) * CP].view(2 * B, H + 1, W + 3, CP)[:, :H, :W, :C].permute(0, 3, 1, 2)
    s = view.stride()
    assert len(set(s)) == 4 and all(a != b for a, b in zip(s, (C * H * W, H * W, W, 1))), s
    assert torch.equal(view.cpu(), val)
    return view


def make_state(shape, dev, seed=0):
    g = torch.Generator().manual_seed(7 + 1000 * seed + shape[0] + 3 * shape[3])
    x, hist, noise = (torch.randn(*shape, generator=g) * s for s in (1.5, 1.0, 1.0))
    return x.to(dev), hist.to(dev), noise.to(dev)


def launch(eps, x, hist, noise, coef, t_next=421, want_x_in=True, want_t_in=True):
    """-> (x', hist', x_in, t_in) of one launch on copies of x / hist; x_in starts as NaN and t_in as -7"""
    B, C, H, W = x.shape
    x, hist = x.clone(), (hist.clone() if hist is not None else None)
    x_in = torch.full((2 * B, C, H, W), float("nan"), dtype=f16, device=x.device) if want_x_in else None
    t_in = torch.full((1,), -7, dtype=torch.int64, device=x.device) if want_t_in else None
    K.sampler_step(eps, x, hist, noise, x_in, t_in, t_next, coef)
    return x, hist, x_in, t_in


def reference(eps, x, hist, noise, coef):
    """the three lines in fp64 on the CPU, with the bounds' S: -> (x' ref, S of x', x0 ref, S of x0)"""
    k = {n: float(coef[n]) for n in COEF_NAMES}
    B = x.shape[0]
    e64 = eps.detach().cpu().to(f64)
    eu, ec = e64[:B], e64[B:]
    xd = x.detach().cpu().to(f64)
    hd = hist.detach().cpu().to(f64) if (hist is not None and k["k_h"] != 0) else torch.zeros_like(xd)
    nd = noise.detach().cpu().to(f64) if (noise is not None and k["k_n"] != 0) else torch.zeros_like(xd)
    e = eu + k["guidance"] * (ec - eu)
    E = eu.abs() + abs(k["guidance"]) * (ec.abs() + eu.abs())
    x0 = k["x0_x"] * xd + k["x0_e"] * e
    S0 = (k["x0_x"] * xd).abs() + abs(k["x0_e"]) * E
    xn = k["k_x"] * xd + k["k_x0"] * x0 + k["k_h"] * hd + k["k_e"] * e + k["k_n"] * nd
    S = (k["k_x"] * xd).abs() + abs(k["k_x0"]) * S0 + (k["k_h"] * hd).abs() + abs(k["k_e"]) * E + (k["k_n"] * nd).abs()
    return xn, S, x0, S0


def within(out, ref, S, what):
    """the elementwise limit; returns the worst |out - ref| / (2^-24 S) (to be at most ROUNDINGS)"""
    out = out.detach().cpu().to(f64)
    assert torch.isfinite(out).all(), f"{what}: not finite (padding or a NaN operand was read)"
    err = (out - ref).abs()
    worst = float((err / (U * S).clamp_min(1e-300)).max())
    assert bool((err <= ROUNDINGS * U * S).all()), f"{what}: worst error {worst:.2f} * 2^-24 * S, limit {ROUNDINGS}"
    return worst


def check_step(shape, layout, name, dev):
    """one launch of coefficient set `name` against the fp64 form, with the required equalities"""
    coef = coef_sets()[name]
    eps = make_eps(shape, layout, dev)
    x, hist, noise = make_state(shape, dev)
    xo, ho, x_in, t_in = launch(eps, x, hist, noise, coef, t_next=421)
    xr, S, x0r, S0 = reference(eps, x, hist, noise, coef)
    wx = within(xo, xr, S, f"x' {shape} {layout} {name}")
    wh = within(ho, x0r, S0, f"hist {shape} {layout} {name}")
    print(f"SAMPLER_STEP {shape} {layout} {name}: worst x' {wx:.2f}, hist {wh:.2f} (* 2^-24 * S, limit {ROUNDINGS})")
    B = shape[0]
    want = xo.half()
    assert torch.equal(x_in[:B].view(torch.int16), want.view(torch.int16)), "x_in's uncond half is not the fp16 of the stored state"
    assert torch.equal(x_in[B:].view(torch.int16), want.view(torch.int16)), "x_in's cond half is not the fp16 of the stored state"
    assert int(t_in) == 421, f"t_in {int(t_in)} is not t_next"
    assert float((xo - x).abs().max()) > 0
    return wx, wh


def check_properties(shape, layout, dev):
    sets = coef_sets()
    eps = make_eps(shape, layout, dev, seed=1)
    x, hist, noise = make_state(shape, dev, seed=1)
    nan = torch.full_like(x, float("nan"))
    # k_n = 0: noise = NULL and a noise tensor of NaNs give the same bits
    a = launch(eps, x, hist, None, sets["dpm_second"])
    b = launch(eps, x, hist, nan, sets["dpm_second"])
    for u, v, what in zip(a, b, ("x'", "hist", "x_in", "t_in")):
        assert torch.equal(u, v), f"k_n = 0: {what} differs between noise = NULL and a NaN noise tensor"
    assert torch.isfinite(a[0]).all()
    # k_h = 0: a NaN hist is never read, and still receives x0
    c = launch(eps, x, nan, noise, sets["ddim_eta1"])
    xr, S, x0r, S0 = reference(eps, x, None, noise, sets["ddim_eta1"])
    within(c[0], xr, S, "x' with k_h = 0 and a NaN hist")
    within(c[1], x0r, S0, "hist (k_h = 0): not overwritten with x0")
    d = launch(eps, x, None, noise, sets["ddim_eta1"])
    assert d[1] is None and torch.equal(d[0], c[0]) and torch.equal(d[2], c[2]), "hist = NULL changes the step"
    # NULL x_in / t_in
    e = launch(eps, x, hist, noise, sets["ddim_eta1"], want_x_in=False, want_t_in=False)
    assert e[2] is None and e[3] is None and torch.equal(e[0], c[0]), "x_in = t_in = NULL changes the state"
    f = launch(eps, x, hist, noise, sets["ddim_eta1"], want_x_in=True, want_t_in=False)
    assert torch.equal(f[2], c[2])
    # a repeat launch
    again = launch(eps, x, nan, noise, sets["ddim_eta1"])
    for u, v, what in zip(c, again, ("x'", "hist", "x_in", "t_in")):
        assert torch.equal(u, v), f"a repeat launch is not bit-identical in {what}"
    # a view whose pixels are not 8-byte aligned takes the path without the one-load form: same bits
    if layout == "nhwc_padded":
        odd = make_eps(shape, layout, dev, seed=1, offset=1)
        assert odd.data_ptr() % 8 != 0 and torch.equal(odd, eps)
        g = launch(odd, x, nan, noise, sets["ddim_eta1"])
        for u, v, what in zip(c, g, ("x'", "hist", "x_in", "t_in")):
            assert torch.equal(u, v), f"{what} depends on the alignment of eps"


def raw_status(eps_t, x_t, coef_set, **over):
    """the library call's return code, with single arguments replaced (None = NULL)"""
    import ctypes as C
    B, Cc, H, W = x_t.shape
    k = capi.SamplerCoef(*(float(coef_set[n]) for n in COEF_NAMES))
    s = eps_t.stride()
    a = dict(eps=eps_t.data_ptr(), es_n=s[0], es_c=s[1], es_h=s[2], es_w=s[3], x=x_t.data_ptr(), hist=None, noise=None, x_in=None, t_in=None,
             t_next=0, B=B, C=Cc, H=H, W=W, coef=C.byref(k))
    a.update(over)
    return capi.lib().cdll.clora_sampler_step_f16(*a.values(), capi.stream())


def check_argument_errors(dev):
    import pytest
    sets = coef_sets()
    shape = (1, 4, 8, 8)
    eps = make_eps(shape, "nchw", dev)
    x, hist, noise = make_state(shape, dev)
    kept = x.clone()
    assert raw_status(eps, x.clone(), sets["ddim_eta0"]) == capi.OK
    bad = [dict(eps=None), dict(x=None), dict(coef=None), dict(B=0), dict(C=0), dict(H=0), dict(W=0), dict(B=-1),
           dict(es_n=0), dict(es_c=0), dict(es_h=0), dict(es_w=0)]
    for over in bad:
        assert raw_status(eps, x, sets["ddim_eta0"], **over) == capi.ERR_ARG, f"{over} must be CLORA_ERR_ARG"
    assert raw_status(eps, x, sets["ddim_eta1"]) == capi.ERR_ARG, "k_n != 0 with noise = NULL must be CLORA_ERR_ARG"
    assert torch.equal(x, kept), "a refused call wrote the state"
    with pytest.raises(capi.CloraError, match="bad argument"):
        K.sampler_step(eps, x, None, None, None, None, 0, sets["ddim_eta1"])
    # what never reaches the library: dtypes, shapes, density
    with pytest.raises(capi.CloraError):
        K.sampler_step(eps, x.half(), None, None, None, None, 0, sets["ddim_eta0"])
    with pytest.raises(capi.CloraError):
        K.sampler_step(eps.float(), x, None, None, None, None, 0, sets["ddim_eta0"])
    with pytest.raises(capi.CloraError):
        K.sampler_step(eps, x.permute(0, 1, 3, 2), None, None, None, None, 0, sets["ddim_eta0"])
    with pytest.raises(capi.CloraError):
        K.sampler_step(eps[:1], x, None, None, None, None, 0, sets["ddim_eta0"])
    with pytest.raises(capi.CloraError):
        K.sampler_step(eps, x, None, None, torch.zeros(2, 4, 8, 8, dtype=f32, device=x.device), None, 0, sets["ddim_eta0"])
    with pytest.raises(capi.CloraError):
        K.sampler_step(eps, x, None, None, None, torch.zeros(1, dtype=torch.int32, device=x.device), 0, sets["ddim_eta0"])
    with pytest.raises(capi.CloraError):
        K.sampler_step(eps, x, None, None, None, None, 0, [1.0, 2.0])
    assert torch.equal(x, kept)


# ------------------------------------------------------------------------------------------------ the loop
class StubUNet:
    """an eps model for the loop on the emulator: each half is fp16 of factor * x * cos(t / 100), with another factor per half"""

    def __call__(self, x_in, t, ehs):
        from types import SimpleNamespace
        B = x_in.shape[0] // 2
        c = torch.cos(torch.as_tensor(t, dtype=f32).reshape(-1)[0] / 100.0)
        out = torch.cat([0.5 * x_in[:B].float() * c, -0.3 * x_in[B:].float() * c + 0.05], 0)
        return SimpleNamespace(sample=out.half())


class Recorder:
    """wraps an eps model: keeps the input and the timestep of every evaluation (the device loop's x_in and t_in)"""

    def __init__(self, model):
        self.model, self.calls = model, []

    def __call__(self, x_in, t, ehs):
        self.calls.append((x_in.detach().clone(), int(torch.as_tensor(t).reshape(-1)[0])))
        return self.model(x_in, t, ehs)


LOOPS = {"ddim8": dict(sampler="ddim", steps=8), "ddim8_eta": dict(sampler="ddim", steps=8, eta=0.7),
         "dpm8": dict(sampler="dpm", steps=8), "dpm20": dict(sampler="dpm", steps=20)}
GUIDANCE = 7.5


def loop_noise(cfg, latents):
    if not cfg.get("eta"):
        return None
    g = torch.Generator().manual_seed(99)
    return torch.randn(cfg["steps"], *latents.shape, generator=g).to(latents.device)


def run_loop(name, unet, control, guide, cond, uncond, latents, graph=False, step_impl="device", record=False, **extra):
    """-> (final latents, [(latents_i, eps_i)] clones recorded through the callback)"""
    from controllora_amd.pipeline import ddim_sample
    cfg = dict(LOOPS[name])
    traj = []
    cb = (lambda i, lat, eps: traj.append((lat.detach().clone(), eps.detach().clone()))) if record else None
    out = ddim_sample(unet, control, guide, cond, uncond, guidance_scale=GUIDANCE, latents=latents, graph=graph, step_impl=step_impl,
                      noise=loop_noise(cfg, latents), callback=cb, **cfg, **extra)
    return out.clone(), traj


def check_teacher_forced(name, unet, control, guide, cond, uncond, latents):
    """an eager device-path run, step by step: the model saw the fp16 of the previous state in both halves and the step's timestep;
    the fp64 host step on the recorded latents_{i-1}, eps_i, noise_i gives the recorded latents_i within the kernel's limit"""
    cfg = LOOPS[name]
    rec = Recorder(unet)
    kept = latents.clone()
    final, traj = run_loop(name, rec, control, guide, cond, uncond, latents, graph=False, record=True)
    assert torch.equal(latents, kept), "the caller's latents were updated in place"
    sched = DDIMScheduler() if cfg["sampler"] == "ddim" else DPMSolverMultistepScheduler()
    sched.set_timesteps(cfg["steps"])
    noise = loop_noise(cfg, latents)
    assert len(traj) == len(rec.calls) == cfg["steps"], "one UNet evaluation and one callback per step"
    assert torch.equal(traj[-1][0], final)
    B = latents.shape[0]
    prev = latents.float()
    orders, worst = [], 0.0
    for i, t in enumerate(sched.timesteps):
        x_seen, t_seen = rec.calls[i]
        assert t_seen == t, f"step {i + 1}: the UNet saw timestep {t_seen}, the schedule says {t}"
        assert torch.equal(x_seen[:B], prev.half()) and torch.equal(x_seen[B:], prev.half()), f"step {i + 1}: the UNet input is not the fp16 of the state"
        lat_i, eps_i = traj[i]
        e64 = eps_i.detach().cpu().to(f64)
        e = e64[:B] + GUIDANCE * (e64[B:] - e64[:B])
        if cfg["sampler"] == "ddim":
            coef = sched.coefficients(i, GUIDANCE, cfg.get("eta", 0.0))
            nz = noise[i].cpu().to(f64) if noise is not None else None
            ref = sched.step(e, t, prev.cpu().to(f64), eta=cfg.get("eta", 0.0), noise=nz)
            hist = None
        else:
            coef = sched.coefficients(i, GUIDANCE)
            hist = sched._x0_hist[-1].clone() if sched._x0_hist else None
            nz = None
            ref = sched.step(e, t, prev.cpu().to(f64))
            orders.append(1 if coef["k_h"] == 0 else 2)
        assert ref.dtype == f64
        _, S, _, _ = reference(eps_i, prev, hist, nz, coef)
        worst = max(worst, within(lat_i, ref, S, f"{name} step {i + 1}"))
        prev = lat_i
    print(f"SAMPLER_LOOP {name}: worst teacher-forced step error {worst:.2f} * 2^-24 * S (limit {ROUNDINGS}), DPM orders {orders}")
    if name == "dpm8":
        assert orders == [1, 2, 2, 2, 2, 2, 2, 1], orders          # lower_order_final: fewer than 15 steps
    if name == "dpm20":
        assert orders == [1] + [2] * 19, orders
    return final
