"""Inference call pattern of the path (reference apps/gradio_canny2image.py:66-92):
hint-encode the guide once (the processors keep the control states across scheduler steps), then a
scheduler loop with classifier-free guidance (UNet batch 2x).  VAE decode / CLIP are outside the hot path
 -- this returns denoised latents."""
from __future__ import annotations

import torch

from .schedulers import DDIMScheduler, DPMSolverMultistepScheduler


@torch.no_grad()
def ddim_sample(unet, control_lora, guide, cond_emb, uncond_emb, steps=50, guidance_scale=9.0, latents=None,
                generator=None, sampler="ddim", graph=None, cache_text_kv=True, callback=None, size=None, eta=0.0, noise=None,
                step_impl="host"):
    """guide [Bc,3,H,W] (control batch 1 broadcasts over the CFG batch, quirk C6); cond/uncond [B,77,768].
    control_lora / guide may be equal-length lists: the main model (whose processors sit on the UNet) first, then the models
    chained onto it with models.mix_control_loras, each with the guide it reads.
    sampler: "ddim" (BASELINE inference config) or "dpm" (DPM-Solver++(2M), what the reference apps select).

    What is invariant over the scheduler loop is evaluated ONCE: the hint encoder and the 32 control terms (reference
    apps/gradio_canny2image.py:84 -- the processors keep the control states), and with `cache_text_kv` the cross-attention
    K/V projections of the text embedding with their adapters (16 sites; they depend on neither the latents nor the
    timestep).  graph: replay ONE captured hipGraph of the UNet forward per step (default: on a GPU); the timestep lives
    in a device tensor, so all steps replay the same graph (default: on a GPU when steps >= 8).
    callback(i, latents, eps): called after scheduler step i = 1..steps (tests record the trajectory with it).
    Without a control model (`control_lora=None`, plain text-to-image) `guide` may be None: `size` = (height, width) of the image
    in pixels, or `latents`, then gives the latent size.
    eta: DDIM's stochastic family (0: deterministic, 1: the DDPM variance).  With eta > 0 step i takes `noise[i - 1]` when `noise`
    ([steps,B,4,H,W], standard normal) is given, else one `torch.randn(..., generator=generator)` draw per step.  With
    sampler="dpm" eta is ignored, as in the reference (its DPM-Solver++ scheduler has no such parameter).
    step_impl: "host" -- the guidance combine and the scheduler update are torch ops on the latents (schedulers `step`);
    "device" -- after each UNet evaluation, eager or replayed, ONE kernels.sampler_step launch on the current stream does both and
    writes the next UNet input and timestep; the coefficients go by value (schedulers `coefficients`).  On the device path the
    callback's `latents` is the in-place state, valid until the next step.
    Returns the denoised latents in **fp32** (the scheduler state is kept in fp32 between steps)."""
    from . import models
    if step_impl not in ("host", "device"):
        raise ValueError(f"step_impl {step_impl!r}: expected 'host' or 'device'")
    if sampler != "ddim":
        eta = 0.0
    eta = float(eta)
    B = cond_emb.shape[0]
    dev = cond_emb.device
    # several control models steering one image (models.mix_control_loras): equal-length lists, the main model first
    many = isinstance(control_lora, (list, tuple))
    if many or isinstance(guide, (list, tuple)):
        control_loras = list(control_lora) if many else [control_lora]
        guides = list(guide) if isinstance(guide, (list, tuple)) else [guide]
        if len(control_loras) != len(guides) or not control_loras or any(c is None for c in control_loras) or \
                any(g is None for g in guides):
            raise ValueError(f"{len(control_loras)} control models and {len(guides)} guide images: every control model needs a guide of its own")
        if len({tuple(g.shape[2:]) for g in guides}) != 1:
            raise ValueError(f"the guides must share one size, got {[tuple(g.shape[2:]) for g in guides]}")
        control_lora, guide = control_loras[0], guides[0]
    else:
        control_loras, guides = [control_lora], [guide]
    if guide is not None:
        H, W = guide.shape[2] // 8, guide.shape[3] // 8
    elif control_lora is not None:
        raise ValueError("a control model needs a guide image")
    elif latents is not None:
        H, W = latents.shape[2], latents.shape[3]
    elif size is not None:
        H, W = int(size[0]) // 8, int(size[1]) // 8
    else:
        raise ValueError("without a guide, give the image size (size=(height, width)) or the initial latents")
    sched = DDIMScheduler() if sampler == "ddim" else DPMSolverMultistepScheduler()
    sched.set_timesteps(steps)
    if latents is None:
        latents = torch.randn((B, 4, H, W), device=dev, dtype=torch.float16, generator=generator) * sched.init_noise_sigma
    # the scheduler state stays fp32 between steps (16 KB per image): only the UNet input is rounded to fp16, so the
    # 50 updates do not each add an fp16 rounding of the latents (denoised-latent parity, tests/full_cases.py)
    latents = latents.float()
    if control_lora is not None:
        # validated ONCE here (the per-site check in models._control_tokens is bypassed by precomputed control terms): a
        # control batch of 1 broadcasts; one guide per image is tiled the way the CFG batch is (uncond..., cond...), which
        # makes the batches equal; anything else has no defined pairing (reference quirk C6) and is rejected
        tiled = []
        for gd in guides:
            if gd.shape[0] == B and B > 1:
                gd = torch.cat([gd, gd], 0)
            elif gd.shape[0] not in (1, 2 * B):
                raise ValueError(f"guide batch {gd.shape[0]}: expected 1 (broadcast) or one guide per image ({B})")
            tiled.append(gd)
        # every model's hint encoder once; the chained members first, so that the main model's forward already sees a chain that
        # folds and evaluates its sites' control terms for the fused path
        for model, gd in reversed(list(zip(control_loras, tiled))):
            model(gd)
    ehs = torch.cat([uncond_emb, cond_emb], 0).half().contiguous()
    if graph is None:
        # capture costs one extra warm-up forward + the capture itself: only worth it for real sampling runs
        graph = dev.type == "cuda" and steps >= 8
    if noise is not None and eta and tuple(noise.shape) != (steps, B, 4, H, W):
        raise ValueError(f"noise {tuple(noise.shape)}: expected one standard-normal tensor per step, {(steps, B, 4, H, W)}")

    def step_noise(i):                                   # the noise of step i = 1..steps: None unless eta > 0
        if not eta:
            return None
        if noise is not None:
            return noise[i - 1].to(device=dev, dtype=torch.float32).contiguous()
        return torch.randn((B, 4, H, W), device=dev, dtype=torch.float32, generator=generator)

    step_kw = (lambda i: dict(eta=eta, noise=step_noise(i))) if eta else (lambda i: {})
    with models.text_kv_cache(enabled=cache_text_kv):
        if step_impl == "device":
            return _device_steps(unet, sched, ehs, latents, guidance_scale, eta, step_noise, graph, callback)
        if not graph:
            for i, t in enumerate(sched.timesteps, 1):
                eps = unet(torch.cat([latents, latents], 0).half(), t, ehs).sample
                eps_u, eps_c = eps.float().chunk(2)
                latents = sched.step(eps_u + guidance_scale * (eps_c - eps_u), t, latents, **step_kw(i))
                if callback is not None:
                    callback(i, latents, eps)
            return latents
        x_in = torch.empty((2 * B, 4, H, W), device=dev, dtype=torch.float16)
        t_in = torch.zeros(1, device=dev, dtype=torch.long)
        x_in.copy_(torch.cat([latents, latents], 0))
        t_in.fill_(int(sched.timesteps[0]))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                # warm-up outside the capture: lazy weight packs, K/V cache, allocator
            unet(x_in, t_in, ehs)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eps_out = unet(x_in, t_in, ehs).sample
        for i, t in enumerate(sched.timesteps, 1):
            x_in.copy_(torch.cat([latents, latents], 0))
            t_in.fill_(int(t))
            g.replay()
            eps_u, eps_c = eps_out.float().chunk(2)
            latents = sched.step(eps_u + guidance_scale * (eps_c - eps_u), t, latents, **step_kw(i))
            if callback is not None:
                callback(i, latents, eps_out)
        return latents


def _device_steps(unet, sched, ehs, latents, guidance_scale, eta, step_noise, graph, callback):
    """The loop of ddim_sample(step_impl="device"): the fp32 state `x`, the previous x0 `hist` (DPM-Solver++ only), the UNet input
    `x_in` and its timestep `t_in` live on the device; one kernels.sampler_step launch per step updates all four."""
    from . import kernels as K
    dev = latents.device
    B = latents.shape[0]
    ddim = isinstance(sched, DDIMScheduler)
    ts = list(sched.timesteps)
    x = latents.float().contiguous().clone()             # updated in place: never the caller's tensor
    hist = None if ddim else torch.zeros_like(x)
    x_in = torch.cat([x, x], 0).half()
    t_in = torch.full((1,), int(ts[0]), device=dev, dtype=torch.long)
    g = None
    if graph:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                # warm-up outside the capture: lazy weight packs, K/V cache, allocator
            unet(x_in, t_in, ehs)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eps = unet(x_in, t_in, ehs).sample
    for i, t in enumerate(ts, 1):
        coef = sched.coefficients(i - 1, guidance_scale, eta) if ddim else sched.coefficients(i - 1, guidance_scale)
        nz = step_noise(i)
        if g is not None:
            g.replay()
        else:
            eps = unet(x_in, t_in, ehs).sample
        K.sampler_step(eps, x, hist, nz, x_in, t_in, ts[i] if i < len(ts) else 0, coef)
        if callback is not None:
            callback(i, x, eps)
    return x


class ControlLoRAPipeline:
    """The `process()` body of the reference apps (apps/gradio_canny2image.py:66-92) without the UI and the annotator:
    prompt(s) + one guide image -> images.  Text encode (cond / negative), hint-encode the guide ONCE (control batch 1 is
    broadcast over the CFG batch, quirk C6), DDIM loop with classifier-free guidance on the HIP UNet, VAE decode.

        pipe = ControlLoRAPipeline.from_pretrained("random:sd15", "path/to/control_lora")
        images = pipe("a red circle", guide, num_samples=4, ddim_steps=50, scale=9.0, seed=1)   # uint8 [N, H, W, 3]

    Several control models (canny + pose): `from_pretrained(base, [main, member, ...])` chains the members onto the main model
    (models.mix_control_loras; fold=False keeps the unfused path) and `pipe(prompt, guide=[g_main, g_member, ...])`.
    """

    def __init__(self, unet, control_lora, vae, text_encoder, tokenizer):
        self.unet, self.control_lora, self.vae, self.text_encoder, self.tokenizer = unet, control_lora, vae, text_encoder, tokenizer

    @classmethod
    def from_pretrained(cls, base: str, control_lora, device="cuda", fold=True):
        from . import loading, models, text
        dev = torch.device(device)
        unet = loading.load_unet(base, dev)
        if isinstance(control_lora, (list, tuple)):    # [main, member, ...]: several guides steer one image
            loaded = [(models.ControlLoRA.from_pretrained(c) if isinstance(c, str) else c).to(dev) for c in control_lora]
            if not loaded:
                raise ValueError("an empty list of control models")
            if len(loaded) == 1:
                unet.set_attn_processor(models.map_processors_to_unet(unet, loaded[0]))
            else:
                models.mix_control_loras(unet, loaded[0], loaded[1:], pre=True, post=False, fold=fold)
            return cls(unet, loaded, loading.load_vae(base, dev), text.load_text_encoder(base, dev, small=base.endswith("small")),
                       text.load_tokenizer(base))
        if isinstance(control_lora, str):
            control_lora = models.ControlLoRA.from_pretrained(control_lora)
        if control_lora is not None:                   # None: the frozen base model alone, plain text-to-image
            control_lora = control_lora.to(dev)
            unet.set_attn_processor(models.map_processors_to_unet(unet, control_lora))
        return cls(unet, control_lora, loading.load_vae(base, dev), text.load_text_encoder(base, dev, small=base.endswith("small")),
                   text.load_tokenizer(base))

    @torch.no_grad()
    def encode_prompt(self, prompts):
        dev = next(self.text_encoder.parameters()).device
        return self.text_encoder(self.tokenizer(list(prompts)).to(dev))[0].half()

    @torch.no_grad()
    def __call__(self, prompt, guide=None, a_prompt="", n_prompt="", num_samples=1, ddim_steps=50, scale=9.0, seed=None,
                 output_type="uint8", sampler="ddim", height=None, width=None, eta=0.0, step_impl="host"):
        """guide: float tensor [1, 3, H, W] (broadcast over the samples) or [num_samples, 3, H, W] (one guide per image), in
        [-1, 1]; H, W multiples of 64, square or not -- every size the reference apps' image_resolution slider gives (256 ... 768):
        the UNet's and the VAE's attention are flash kernels that take any number of tokens.  A pipeline built from a list of control
        models ([main, member, ...]) takes a list of guides, one per model in that order, all of one size.
        A pipeline without a control model takes no guide: `height` / `width` (multiples of 64, default 512) size the image.
        eta / step_impl: see ddim_sample (eta is DDIM's; step_impl "device" runs each scheduler step as one launch)."""
        if guide is None:
            if self.control_lora is not None:
                raise ValueError("this pipeline has a control model: it needs a guide image")
            height, width = int(height or width or 512), int(width or height or 512)
            if height % 64 or width % 64:
                raise ValueError(f"height / width must be multiples of 64, got {height} x {width}")
        dev = next(self.text_encoder.parameters()).device
        gen = torch.Generator(device=dev)
        if seed is not None:
            gen.manual_seed(int(seed))
        cond = self.encode_prompt([prompt + (", " + a_prompt if a_prompt else "")] * num_samples)
        uncond = self.encode_prompt([n_prompt] * num_samples)
        if isinstance(guide, (list, tuple)):
            guide = [g.to(dev).half() for g in guide]
        elif guide is not None:
            guide = guide.to(dev).half()
            if isinstance(self.control_lora, (list, tuple)):
                guide = [guide]                        # (a list of one model takes a bare guide too)
        lat = ddim_sample(self.unet, self.control_lora, guide, cond, uncond,
                          steps=ddim_steps, guidance_scale=scale, generator=gen, sampler=sampler,
                          size=None if guide is not None else (height, width), eta=eta, step_impl=step_impl)
        img = self.vae.decode(lat.half() / self.vae.scaling_factor).sample.float().clamp(-1, 1)
        if output_type == "uint8":
            return ((img.permute(0, 2, 3, 1) + 1.0) * 127.5).round().to(torch.uint8).cpu()
        return img
