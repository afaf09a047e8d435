"""Shared cases of the DreamBooth-LoRA tests (CPU on the emulated kernels, GPU on the real library): the per-sample-weighted
MSE launch (clora_mse_weighted_f16) against clora_mse_f16 and an fp64 formula, and one prior-preservation train step of the
plain-LoRA trainer against the oracle UNet with autograd (the reference's loss, train_dreambooth_lora.py:898-910)."""
import functools
import os

import torch
from safetensors.torch import load_file

from controllora_amd import capi, kernels as K
from controllora_amd.train import AttnProcsLayers, LoRATrainer
from oracle import cases, unet_ref
from tests.e2e_cases import build_product_case, rel

f16, f32 = torch.float16, torch.float32

# (B, n_per_sample): one vector; every lane of a wave in another sample; the tests' 16x16 latent; the 512x512 latent at the
# reference's batch 4 + 4 (two blocks per sample); sample boundaries that fall mid-wave and mid-block of the flat tensor
KERNEL_SHAPES = [(1, 8), (4, 8), (3, 4 * 16 * 16), (8, 4 * 64 * 64), (5, 8 * 1001)]
LOSS_SCALE = 1024.0
TOL_SEED = 6e-4       # one fp16 rounding per element (the limit case_loss_and_optimizer uses for clora_mse_f16's seed)
TOL_SUM = 1e-4        # fp32 sums whose serial chains stay short, against the fp64 sum of the same fp16 inputs
# the `lora` case's limits in tests/e2e_cases.check_against_golden
TOL_PRED, TOL_GRAD, TOL_LOSS = 5e-3, 2.5e-2, 2e-3
PRIOR_WEIGHT = 0.25   # not 1: with 1 the loss is twice the plain mean and a kernel that ignores the weights would pass


# ------------------------------------------------------------------------------------------------ kernel
def kernel_inputs(B, n, dev, seed=0):
    g = torch.Generator().manual_seed(seed + 17 * B + n)
    pred = torch.randn(B, n, generator=g).half().to(dev)
    target = torch.randn(B, n, generator=g).half().to(dev)
    return pred, target


def mixed_weights(B, dev):
    return torch.tensor(([1.0, 0.25, 0.0, 2.0, 0.5, 1.5, 0.0, 3.0] * (B // 8 + 1))[:B], dtype=f32, device=dev)


def run_weighted(pred, target, weights, grad_scale, scale, with_dpred=True):
    B = pred.shape[0]
    sums = torch.zeros(B, dtype=f32, device=pred.device)
    dpred = torch.full_like(pred, float("nan")) if with_dpred else None
    K.mse_weighted(pred, target, weights, sums, dpred, grad_scale, scale)
    return sums, dpred


def check_unit_weights_equal_plain_mse(B, n, dev):
    """all weights 1: the seed is clora_mse_f16's bit for bit, and the per-sample sums add up to its loss sum"""
    pred, target = kernel_inputs(B, n, dev)
    scale = torch.tensor([LOSS_SCALE], dtype=f32, device=dev)
    gs = 2.0 / (B * n)
    loss_sum = torch.zeros(1, dtype=f32, device=dev)
    ref = torch.full_like(pred, float("nan"))
    K.mse(pred.reshape(-1), target.reshape(-1), loss_sum, ref.reshape(-1), gs, scale)
    sums, dpred = run_weighted(pred, target, torch.ones(B, dtype=f32, device=dev), gs, scale)
    total, plain = float(sums.double().sum()), float(loss_sum)
    print(f"MSE_WEIGHTED unit weights ({B}, {n}): sum of sample sums {total!r} vs clora_mse_f16 {plain!r} "
          f"(rel {abs(total - plain) / plain:.2e}, limit 1e-6)")
    assert torch.equal(dpred, ref), "with every weight 1.0 the seed must be clora_mse_f16's, bit for bit"
    assert abs(total - plain) <= 1e-6 * plain
    return total, plain


def check_mixed_weights_against_fp64(B, n, dev):
    pred, target = kernel_inputs(B, n, dev, seed=1)
    scale = torch.tensor([LOSS_SCALE], dtype=f32, device=dev)
    w = mixed_weights(B, dev)
    gs = 2.0 / n
    sums, dpred = run_weighted(pred, target, w, gs, scale)
    d = pred.double().cpu() - target.double().cpu()
    ref_seed = float(torch.tensor(gs, dtype=f32)) * LOSS_SCALE * w.double().cpu()[:, None] * d
    ref_sums = (d * d).sum(1)
    e_seed = rel(dpred.double().cpu(), ref_seed) if float(ref_seed.norm()) > 0 else float(dpred.float().abs().max())
    e_sums = ((sums.double().cpu() - ref_sums).abs() / ref_sums).max()
    print(f"MSE_WEIGHTED mixed weights ({B}, {n}): seed rel-L2 {e_seed:.3e} (limit {TOL_SEED}), worst sample sum rel {float(e_sums):.3e} "
          f"(limit {TOL_SUM})")
    assert torch.isfinite(dpred.float()).all()
    assert e_seed < TOL_SEED
    for b in range(B):
        if float(w[b]) == 0.0:
            assert not bool(dpred[b].float().abs().max() > 0), f"sample {b} has weight 0: its seed must be exactly zero"
        else:
            assert float(dpred[b].float().abs().max()) > 0
    assert float(e_sums) < TOL_SUM
    # loss only: the same sums, nothing written anywhere else
    sums_only, none = run_weighted(pred, target, w, gs, scale, with_dpred=False)
    assert none is None and torch.equal(sums_only, sums), "dpred = NULL must leave the sums identical"
    # a repeat launch on re-zeroed sums
    sums2, dpred2 = run_weighted(pred, target, w, gs, scale)
    assert torch.equal(dpred2, dpred), "a repeat launch is not bit-identical"
    assert torch.equal(sums2, sums)
    # the sums are accumulated into, not overwritten
    K.mse_weighted(pred, target, w, sums2, None, gs, scale)
    assert rel(sums2, 2 * sums) < 1e-6
    return e_seed, float(e_sums)


def check_argument_errors(dev):
    import pytest
    pred, target = kernel_inputs(1, 16, dev)
    one = torch.ones(1, dtype=f32, device=dev)
    with pytest.raises(capi.CloraError, match="bad argument"):
        K.mse_weighted(pred[:, :12].contiguous(), target[:, :12].contiguous(), one, torch.zeros(1, dtype=f32, device=dev), None, 1.0)
    with pytest.raises(capi.CloraError):                    # weights and sums of different lengths never reach the library
        K.mse_weighted(pred, target, one, torch.zeros(2, dtype=f32, device=dev), None, 1.0)


# ------------------------------------------------------------------------------------------------ trainer step
@functools.lru_cache(maxsize=None)
def oracle_prior_step(weight=PRIOR_WEIGHT):
    """fp32 CPU autograd on the oracle UNet with LoRA processors on every site, batch 4 = [instance, instance, prior, prior]:
    loss = mse(pred[:2], noise[:2]) + weight * mse(pred[2:], noise[2:])  (computed once, shared, never modified)"""
    import torch.nn.functional as F
    inp = cases.seeded_inputs(batch=4)
    unet, params, _ = cases.build_oracle_case("lora")
    for p in unet.parameters():
        p.requires_grad_(False)
    for p in params.parameters():
        p.requires_grad_(True)
        p.grad = None
    noisy = unet_ref.DDPMSchedule().add_noise(inp["latents"], inp["noise"], inp["timesteps"])
    pred = unet(noisy, inp["timesteps"], inp["ehs"]).sample
    inst = F.mse_loss(pred[:2].float(), inp["noise"][:2].float(), reduction="mean")
    prior = F.mse_loss(pred[2:].float(), inp["noise"][2:].float(), reduction="mean")
    loss = inst + weight * prior
    loss.backward()
    return dict(pred=pred.detach(), loss=float(loss.detach()), instance=float(inst.detach()), prior=float(prior.detach()), grads=cases.flat_grads(params).clone())


def make_trainer(dev, **kw):
    unet, _, _ = build_product_case("lora", dev)
    layers = AttnProcsLayers(unet.attn_processors)
    kw.setdefault("init_scale", 128.0)
    kw.setdefault("dynamic_scale", False)
    return LoRATrainer(unet, layers, **kw)


def step_args(dev, batch):
    inp = cases.seeded_inputs(batch=batch)
    noisy = unet_ref.DDPMSchedule().add_noise(inp["latents"], inp["noise"], inp["timesteps"]).to(dev).to(f16)
    return noisy, inp["timesteps"].to(dev), inp["ehs"].to(dev).to(f16), inp["noise"].to(dev)


def prior_weights(dev, weight=PRIOR_WEIGHT):
    return torch.tensor([1.0, 1.0, weight, weight], dtype=f32, device=dev)


def check_prior_preservation_step(dev):
    ref = oracle_prior_step()
    tr = make_trainer(dev)
    pred = tr.forward_backward(*step_args(dev, 4), prior_weights(dev))
    inst, prior = tr.loss_parts()
    errs = {"pred": rel(pred.detach(), ref["pred"]), "grads": rel(tr.unscaled_grads_module_order(), ref["grads"]),
            "loss": abs(tr.loss() - ref["loss"]) / ref["loss"], "instance": abs(inst - ref["instance"]) / ref["instance"],
            "prior": abs(prior - ref["prior"]) / ref["prior"]}
    print("DREAMBOOTH_PRIOR_STEP", {k: f"{v:.3e}" for k, v in errs.items()}, "oracle", {k: ref[k] for k in ("loss", "instance", "prior")})
    # the case tells the weighting apart: the plain mean over the batch (weight 1, divided by 2) is far from the oracle loss
    plain = 0.5 * (ref["instance"] + ref["prior"])
    assert abs(plain - ref["loss"]) / ref["loss"] > 50 * TOL_LOSS
    assert errs["pred"] < TOL_PRED and errs["grads"] < TOL_GRAD and errs["loss"] < TOL_LOSS, errs
    assert errs["instance"] < TOL_LOSS and errs["prior"] < TOL_LOSS, errs
    assert abs(tr.loss() - (inst + PRIOR_WEIGHT * prior)) <= 1e-6 * tr.loss()
    return errs


def check_plain_step_against_golden(dev, golden_dir):
    """sample_weights=None at batch 2: tests/e2e_cases.check_against_golden("lora") through LoRATrainer (no stand-in hint encoder)"""
    gold = load_file(os.path.join(golden_dir, "case_lora.safetensors"))
    tr = make_trainer(dev)
    pred = tr.forward_backward(*step_args(dev, 2))
    errs = {"pred": rel(pred.detach(), gold["pred"]), "grads": rel(tr.unscaled_grads_module_order(), gold["grads"]),
            "loss": rel(torch.tensor([tr.loss(pred.numel())]), gold["loss"])}
    print("DREAMBOOTH_PLAIN_STEP", {k: f"{v:.3e}" for k, v in errs.items()})
    assert errs["pred"] < TOL_PRED and errs["grads"] < TOL_GRAD and errs["loss"] < TOL_LOSS, errs
    assert abs(tr.loss() - tr.loss(pred.numel())) == 0.0
    import pytest
    with pytest.raises(RuntimeError):
        tr.loss_parts()
    return errs
