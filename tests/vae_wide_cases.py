"""The VAE past 8,192 latent tokens and at non-square sizes: the product's VaeAttention (controllora_amd/vae.py: one launch of the
wide flash forward kernel for the whole batch) against oracle/vae_ref.AttentionBlock in fp64, and the whole VAE against the oracle
at H != W (tests/vae_cases.check_vae is square-only).  Weights as tests/vae_cases.py makes them: fp16-representable, non-trivial
norm affine and biases."""
import torch

from controllora_amd import vae as V
from oracle import vae_ref as R

from tests.vae_cases import rel

WIDE_SMALL_VAE = dict(in_channels=3, out_channels=3, latent_channels=4, block_out_channels=(16, 32, 32, 256),
                      layers_per_block=1, norm_num_groups=8)


def _test_weights_(module):
    with torch.no_grad():
        for n, p in module.named_parameters():
            if p.ndim == 1:
                p.copy_((0.2 * torch.randn_like(p) + (1.0 if "norm" in n and n.endswith("weight") else 0.0)))
            p.copy_(p.half().float())


def rel64(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def check_attention_block(dev, batch, th, tw, c=512, groups=32, tol=3e-3):
    """VaeAttention(c, groups) on batch x (th x tw) tokens against the oracle block in fp64 on the same device.  3e-3 norm-wise on the
    block output: the 2e-3 limit of the attention kernel on the branch and five fp16-stored tensors (norm output, q, k, v, block output)
    at the 3-6e-4 the project's error budget measured per stored tensor, in quadrature about 2.4e-3; the residual only dilutes it.
    The materialised-scores path is measured beside the flash path where it can run (printed, and held to the same limit)."""
    torch.manual_seed(5)
    o = R.AttentionBlock(c, groups)
    _test_weights_(o)
    m = V.VaeAttention(c, groups)
    with torch.no_grad():
        sd = o.state_dict()
        for k, p in m.state_dict().items():
            p.copy_(sd[k].reshape(p.shape).to(p.dtype))
    m.to(dev)
    x = torch.randn(batch, c, th, tw).half()
    with torch.no_grad():
        ref = torch.cat([o.double().to(dev)(x[b:b + 1].double().to(dev)) for b in range(batch)])   # one image's scores at a time
    ref = ref.permute(0, 2, 3, 1).reshape(batch, th * tw, c)
    tokens = x.permute(0, 2, 3, 1).reshape(batch, th * tw, c).contiguous().to(dev)
    errs = {}
    for name, flash in (("flash", True), ("scores", False)):
        if not flash and th * tw > V.VaeAttention.SCORES_MAX_TOKENS:
            continue
        m.use_flash = flash                                   # instance attribute: the class default is left alone
        with torch.no_grad():
            out = m(tokens)
        assert out.shape == ref.shape and bool(torch.isfinite(out.float()).all())
        errs[name] = rel64(out, ref)
    print(f"VAE_ATTENTION_BLOCK B={batch} tokens={th}x{tw} C={c} " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < tol, errs
    return errs


def check_vae_rect(dev, height, width, batch=2, cfg=None, tol=6e-3, flash=None):
    """tests/vae_cases.check_vae at height != width: encoder moments, sampled latents and the decoded image against the oracle.
    flash: True / False pins the mid-block attention path (VaeAttention.use_flash) for the call, None leaves the default"""
    if flash is not None:
        old = V.VaeAttention.use_flash
        V.VaeAttention.use_flash = flash
        try:
            return check_vae_rect(dev, height, width, batch, cfg, tol)
        finally:
            V.VaeAttention.use_flash = old
    cfg = WIDE_SMALL_VAE if cfg is None else cfg
    torch.manual_seed(3)
    o = R.AutoencoderKL(**cfg)
    _test_weights_(o)
    m = V.AutoencoderKL(**cfg)
    V.load_from_oracle_(m, o)
    m.to(dev)
    x = (torch.rand(batch, 3, height, width) * 2 - 1).half().float()
    eps = torch.randn(batch, 4, height // 8, width // 8)
    with torch.no_grad():
        mean_o, logvar_o = o.moments(x)
        z_o = o.encode_sample(x, eps)
        img_o = o.decode(z_o.half().float())
    dist = m.encode(x.to(dev).half()).latent_dist
    assert dist.mean.shape == (batch, 4, height // 8, width // 8) and dist.mean.dtype == torch.float32
    errs = {"mean": rel(dist.mean, mean_o), "logvar": rel(dist.logvar, logvar_o)}
    errs["sample"] = rel(dist.sample(noise=eps.to(dev)), z_o)
    img = m.decode(z_o.to(dev).half()).sample
    assert img.shape == (batch, 3, height, width)
    errs["decode"] = rel(img, img_o)
    print(f"VAE_RECT {height}x{width} B={batch} " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < tol, errs
    return errs
