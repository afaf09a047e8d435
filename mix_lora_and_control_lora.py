#!/usr/bin/env python
"""Sample with a plain LoRA (e.g. a DreamBooth one) chained onto a ControlLoRA.

What the reference's mix_lora_and_control_lora.py does with constants edited in the file, as a command line: the LoRA's
processors are injected before and / or after the ControlLoRA processors of every attention site, then each validation image is
sampled with DPM-Solver++ from one guide of the data set and written as `samples/<output_dir>/<i>.png` = [guide | image].

    python mix_lora_and_control_lora.py --pretrained_model_name_or_path random:sd15 --control_lora random:fill50k.json \\
        --lora random:3 --dataset_name synthetic:fill50k --validation_prompt "red circle with blue background"

The frozen LoRA is folded into the frozen attention weights once (one kernel launch for the whole model), so the sampler runs
exactly the launches of the unmixed sampler; `--no_fold` keeps the chained sites on the generic, unfused path."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--pretrained_model_name_or_path", required=True,
                   help="SD-1.5 checkpoint directory (diffusers layout), or random:sd15 / random:small (seeded weights, offline)")
    p.add_argument("--control_lora", required=True,
                   help="directory written by ControlLoRA.save_pretrained, or random:<config file, or its name under configs/> "
                        "(seeded, non-zero adapters)")
    p.add_argument("--lora", required=True,
                   help="diffusers-format LoRA (pytorch_lora_weights.bin, diffusion_pytorch_model.bin, a .safetensors of the same "
                        "dict, or a folder holding one), or random:<seed> for a seeded stand-in with non-zero up matrices")
    p.add_argument("--lora_rank", type=int, default=4, help="rank of a random:<seed> LoRA")
    p.add_argument("--lora_std", type=float, default=0.02, help="weight scale of a random:<seed> LoRA (0 = a LoRA that does nothing)")
    p.add_argument("--dataset_name", default="synthetic:fill50k", help="synthetic:fill50k or a process/<name> data set; only guides are read")
    p.add_argument("--resolution", type=int, default=512)
    p.add_argument("--validation_prompt", required=True)
    p.add_argument("--num_validation_images", type=int, default=16)
    p.add_argument("--inject_pre_lora", dest="inject_pre_lora", action="store_true", default=True)
    p.add_argument("--no_inject_pre_lora", dest="inject_pre_lora", action="store_false")
    p.add_argument("--inject_post_lora", action="store_true", default=False)
    p.add_argument("--num_inference_steps", type=int, default=30)
    p.add_argument("--guidance_scale", type=float, default=7.5, help="the pipeline's default guidance")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--output_dir", default="mix")
    p.add_argument("--no_fold", action="store_true", help="keep chained sites on the generic path (one kernel group per adapter)")
    return p.parse_args(argv)


def load_control_lora(name, dev, seed=1):
    from controllora_amd import models as M
    if not name.startswith("random:"):
        return M.ControlLoRA.from_pretrained(name).to(dev)
    cfg = name.split(":", 1)[1] or "fill50k.json"
    torch.manual_seed(seed)
    clora = M.ControlLoRA.from_config(cfg if os.path.exists(cfg) else os.path.join(ROOT, "configs", cfg))
    with torch.no_grad():                                # trained adapters have non-zero up matrices
        for n, q in clora.named_parameters():
            if ".up.weight" in n:
                q.normal_(0.0, 0.02)
    return clora.to(dev)


def random_lora_state_dict(unet, seed, rank=4, std=0.02):
    """a seeded diffusers-format LoRA state dict for every attention site of `unet`"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name in unet.attn_processors:
        site = unet.get_submodule(name[:-len(".processor")])
        hidden, kv_in = site.to_q.weight.shape[0], site.to_k.weight.shape[1]
        for part, cin in (("q", site.to_q.weight.shape[1]), ("k", kv_in), ("v", kv_in), ("out", hidden)):
            sd[f"{name}.to_{part}_lora.down.weight"] = torch.randn(rank, cin, generator=g) / rank
            sd[f"{name}.to_{part}_lora.up.weight"] = torch.randn(hidden, rank, generator=g) * std
    return sd


def guides(args, tokenizer):
    from controllora_amd import data
    if args.dataset_name.startswith("synthetic:"):
        ds = data.SyntheticFill50k(args.resolution, max(args.num_validation_images, 1), seed=args.seed or 42)
    elif args.dataset_name.startswith("process/"):
        from controllora_amd import process
        ds = process.Dataset.from_name(args.dataset_name)(tokenizer, resolution=args.resolution, use_crop=True)
    else:
        raise ValueError("--dataset_name: synthetic:fill50k or a process/<name> data set")
    for i in range(args.num_validation_images):
        yield ds[i % len(ds)]["guide_values"]


@torch.no_grad()
def main(argv=None):
    args = parse_args(argv)
    from PIL import Image
    from controllora_amd import loading, models as M, text
    from controllora_amd.pipeline import ddim_sample
    if not torch.cuda.is_available():
        raise RuntimeError("sampling runs on the HIP kernels: an MI355X is needed (no CPU fallback is provided)")
    dev = torch.device("cuda")
    name = args.pretrained_model_name_or_path
    tokenizer = text.load_tokenizer(name)
    text_encoder = text.load_text_encoder(name, dev, small=name.endswith("small"))
    vae = loading.load_vae(name, dev)
    unet = loading.load_unet(name, dev)
    control_lora = load_control_lora(args.control_lora, dev)
    if args.lora.startswith("random:"):
        lora = random_lora_state_dict(unet, int(args.lora.split(":", 1)[1] or 0), args.lora_rank, args.lora_std)
    else:
        lora = args.lora
    procs = loading.load_lora_attn_procs(unet, lora)
    M.mix_lora_into_control_lora(unet, control_lora, procs, pre=args.inject_pre_lora, post=args.inject_post_lora, fold=not args.no_fold)
    report = control_lora.fold_report()
    folded = sum(r["folded"] for r in report.values())
    print(f"{len(report)} attention sites mixed (pre={args.inject_pre_lora}, post={args.inject_post_lora}); {folded} run on folded weights"
          + ("" if folded == len(report) else "; the others stay on the generic path: "
             + "; ".join(sorted({r["reason"] for r in report.values() if not r["folded"]}))))
    cond = text_encoder(tokenizer([args.validation_prompt]).to(dev))[0].half()
    uncond = text_encoder(tokenizer([""]).to(dev))[0].half()
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    out_dir = os.path.join("samples", args.output_dir)
    os.makedirs(out_dir, exist_ok=True)
    for i, guide in enumerate(guides(args, tokenizer)):
        lat = ddim_sample(unet, control_lora, guide[None].to(dev).half(), cond, uncond, steps=args.num_inference_steps,
                          guidance_scale=args.guidance_scale, generator=gen, sampler="dpm")
        img = vae.decode(lat.half() / vae.scaling_factor).sample.float().clamp(-1, 1)[0].cpu()
        g = torch.nn.functional.interpolate(guide[None].float(), size=img.shape[1:], mode="bilinear", align_corners=False)[0]
        strip = torch.cat([g.clamp(-1, 1), img], dim=2)                                     # [guide | image]
        arr = ((strip.permute(1, 2, 0).numpy() + 1.0) * 127.5).round().astype(np.uint8)
        Image.fromarray(arr).save(os.path.join(out_dir, f"{i}.png"))
    print(f"wrote {args.num_validation_images} images to {out_dir}")
    return out_dir


if __name__ == "__main__":
    main()
