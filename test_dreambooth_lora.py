#!/usr/bin/env python
"""Turn a `checkpoint-N` of train_dreambooth_lora.py into final LoRA weights and sample with them: the counterpart of the
reference's test_dreambooth_lora.py (:824-885) on the MI355X-native path.  Takes the flags of the training script (its
`parse_args` is reused), loads `--resume_from_checkpoint` (the basename of a path, or `latest`) from `--output_dir` -- a missing
one is logged and the freshly initialised adapters are used, as in the reference --, writes `pytorch_lora_weights.bin` and
`.safetensors` there, then makes `--num_validation_images` samples of `--validation_prompt` without a control model:
DPM-Solver++(2M), 25 steps, guidance 7.5, one generator seeded with `--seed` for all of them, saved as
`samples/<basename of output_dir>/<i>.png`.

    python test_dreambooth_lora.py --pretrained_model_name_or_path random:sd15 --instance_data_dir dog/ \\
        --instance_prompt "a photo of sks dog" --output_dir lora-dog --resume_from_checkpoint latest \\
        --validation_prompt "a photo of sks dog in a bucket" --seed 0

Additions: `--num_inference_steps`, `--sampler_step` (how the scheduler step between two UNet evaluations runs: `device` = one
HIP launch, `host` = torch ops) and `--samples_dir` (where `samples/` lies).
"""
from __future__ import annotations

import argparse
import logging
import os

import torch

import train_dreambooth_lora as T

logger = logging.getLogger("dreambooth_lora.test")


def parse_args(argv=None):
    """the training script's flags (T.parse_args) plus the three of this script"""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--num_inference_steps", type=int, default=25)
    p.add_argument("--sampler_step", type=str, default="device", choices=["host", "device"])
    p.add_argument("--samples_dir", type=str, default="samples")
    own, rest = p.parse_known_args(argv)
    args = T.parse_args(rest)
    for k, v in vars(own).items():
        setattr(args, k, v)
    return args


def resolve_checkpoint(args):
    """-> the checkpoint directory `--resume_from_checkpoint` names inside `--output_dir`, or None (logged) when there is none"""
    want = args.resume_from_checkpoint
    if not want:
        return None
    name = os.path.basename(os.path.normpath(want)) if want != "latest" else T.latest_checkpoint(args.output_dir)
    if name is None or not os.path.isdir(os.path.join(args.output_dir, name)):
        logger.info("Checkpoint '%s' does not exist. Starting a new training run.", want)
        return None
    return os.path.join(args.output_dir, name)


def samples_dir(args):
    return os.path.join(args.samples_dir, os.path.basename(os.path.normpath(args.output_dir)))


@torch.no_grad()
def sample(args, unet, vae, text_encoder, tokenizer, dev):
    import numpy as np
    from PIL import Image
    from controllora_amd.pipeline import ddim_sample
    out_dir = samples_dir(args)
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    if not args.validation_prompt or args.num_validation_images <= 0:
        return paths
    gen = torch.Generator(device=dev)
    if args.seed:                                                  # the reference leaves the generator unseeded without --seed
        gen.manual_seed(args.seed)
    res = -(-args.resolution // 64) * 64
    cond = text_encoder(tokenizer([args.validation_prompt]).to(dev))[0].half()
    uncond = text_encoder(tokenizer([""]).to(dev))[0].half()
    for i in range(args.num_validation_images):
        lat = ddim_sample(unet, None, None, cond, uncond, steps=args.num_inference_steps, guidance_scale=7.5, generator=gen,
                          sampler="dpm", size=(res, res), step_impl=args.sampler_step)
        img = vae.decode(lat.half() / vae.scaling_factor).sample.float().clamp(-1, 1)
        paths.append(os.path.join(out_dir, f"{i}.png"))
        Image.fromarray(((img[0].permute(1, 2, 0).cpu().numpy() + 1.0) * 127.5).round().astype(np.uint8)).save(paths[-1])
    return paths


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(format="%(asctime)s - %(levelname)s - %(name)s - %(message)s", level=logging.INFO)
    from controllora_amd import loading, text
    from controllora_amd.train import AttnProcsLayers, LoRATrainer
    if not torch.cuda.is_available():
        raise RuntimeError("the DreamBooth LoRA path needs an MI355X (no CPU fallback is provided)")
    local = max(args.local_rank, 0)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    name = args.pretrained_model_name_or_path
    tokenizer = T.load_tokenizer(args)
    text_encoder = text.load_text_encoder(name, dev, small=name.endswith("small"))
    vae = loading.load_vae(name, dev)
    unet = loading.load_unet(name, dev)
    unet.set_attn_processor(T.build_lora_processors(unet, args.lora_rank, dev))

    logger.info("***** Running testing *****")
    checkpoint = resolve_checkpoint(args)
    if checkpoint is not None:
        logger.info("Resuming from checkpoint %s", os.path.basename(checkpoint))
        LoRATrainer(unet, AttnProcsLayers(unet.attn_processors)).load_state(checkpoint)

    os.makedirs(args.output_dir, exist_ok=True)
    unet.save_attn_procs(args.output_dir, weights_name=loading.LORA_WEIGHT_NAME, save_function=torch.save)
    unet.save_attn_procs(args.output_dir, weights_name=loading.LORA_WEIGHT_NAME_SAFE, safe_serialization=True)
    logger.info("Saved the LoRA to %s", args.output_dir)

    paths = sample(args, unet, vae, text_encoder, tokenizer, dev)
    logger.info("Saved %d samples to %s", len(paths), samples_dir(args))
    return paths


if __name__ == "__main__":
    main()
