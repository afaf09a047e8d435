#!/usr/bin/env python
"""Turn a `checkpoint-N` of train_text_to_image_control_lora.py into final weights and sample with them: the counterpart of the
reference's test_text_to_image_control_lora.py (:705-790) on the MI355X-native path.  Takes the flags of the training script (its
`parse_args` and `build_dataset` are reused), loads `--resume_from_checkpoint` (the basename of a path, or `latest`) from
`--output_dir`, writes `config.json` and the ControlLoRA weights in both formats there, then samples `--num_validation_images`
images one at a time -- DPM-Solver++(2M), guidance 7.5, ONE generator seeded with `--seed` for all of them, the guides of
consecutive unshuffled data set items -- and saves `samples/<basename of output_dir>/<i>.png` as the data set's `cat_input`
strip [target | guide | image].

    python test_text_to_image_control_lora.py --pretrained_model_name_or_path random:sd15 --dataset_name synthetic:fill50k \\
        --control_lora_config configs/fill50k.json --output_dir sd-fill50k-model-control-lora --resume_from_checkpoint latest \\
        --validation_prompt "pale golden rod circle with old lace background" --seed 0

A checkpoint that is named but missing is a ValueError, as in the reference; without `--resume_from_checkpoint` the freshly
initialised adapters are written and sampled, as there.  Additions: `--num_inference_steps` (the reference samples 30 steps), `--sampler_step` (how the scheduler step between two UNet
evaluations runs: `device` = one HIP launch, `host` = torch ops) and `--samples_dir` (where `samples/` lies).
"""
from __future__ import annotations

import argparse
import logging
import os

import torch

import train_text_to_image_control_lora as T

logger = logging.getLogger("control_lora.test")


def parse_args(argv=None):
    """the training script's flags (T.parse_args) plus the three of this script"""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--num_inference_steps", type=int, default=30)
    p.add_argument("--sampler_step", type=str, default="device", choices=["host", "device"])
    p.add_argument("--samples_dir", type=str, default="samples")
    own, rest = p.parse_known_args(argv)
    args = T.parse_args(rest)
    for k, v in vars(own).items():
        setattr(args, k, v)
    return args


def resolve_checkpoint(args):
    """-> the checkpoint directory `--resume_from_checkpoint` names inside `--output_dir` (None without the flag); ValueError
    when the one it names does not exist"""
    want = args.resume_from_checkpoint
    if not want:
        return None
    name = os.path.basename(os.path.normpath(want)) if want != "latest" else T.latest_checkpoint(args.output_dir)
    if name is None or not os.path.isdir(os.path.join(args.output_dir, name)):
        raise ValueError(f"Checkpoint '{want}' does not exist.")
    return os.path.join(args.output_dir, name)


def samples_dir(args):
    return os.path.join(args.samples_dir, os.path.basename(os.path.normpath(args.output_dir)))


@torch.no_grad()
def sample(args, unet, control_lora, vae, text_encoder, tokenizer, dataset, dev):
    import numpy as np
    from PIL import Image
    from controllora_amd import data, process
    from controllora_amd.pipeline import ddim_sample
    out_dir = samples_dir(args)
    os.makedirs(out_dir, exist_ok=True)
    gen = torch.Generator(device=dev).manual_seed(args.seed or 0)
    cond = text_encoder(tokenizer([args.validation_prompt or ""]).to(dev))[0].half()
    uncond = text_encoder(tokenizer([""]).to(dev))[0].half()
    paths = []
    for i in range(args.num_validation_images):
        ex = dataset[i % len(dataset)]
        if "canny_image" in ex:                                   # --canny_detector device: the item carries no guide yet
            ex["guide_values"] = process.device_guides(data.collate([ex]), dev)["guide_values"][0].float().cpu()
        guide = ex["guide_values"][None].to(dev).half()
        lat = ddim_sample(unet, control_lora, guide, cond, uncond, steps=args.num_inference_steps, guidance_scale=7.5, generator=gen,
                          sampler="dpm", step_impl=args.sampler_step)
        img = vae.decode(lat.half() / vae.scaling_factor).sample.float().clamp(-1, 1)
        image = Image.fromarray(((img[0].permute(1, 2, 0).cpu().numpy() + 1.0) * 127.5).round().astype(np.uint8))
        cat_input = getattr(type(dataset), "cat_input", process.Dataset.cat_input)     # the data set's own strip, else the base one
        strip = cat_input(image, ex["pixel_values"][None], ex["guide_values"][None])
        paths.append(os.path.join(out_dir, f"{i}.png"))
        strip.save(paths[-1])
    return paths


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(format="%(asctime)s - %(levelname)s - %(name)s - %(message)s", level=logging.INFO)
    from controllora_amd import loading, models as M, text
    from controllora_amd.train import ControlLoRATrainer
    if not torch.cuda.is_available():
        raise RuntimeError("the ControlLoRA path needs an MI355X (no CPU fallback is provided)")
    local = max(args.local_rank, 0)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    checkpoint = resolve_checkpoint(args)                          # before anything is loaded: a named but missing one is an error

    name = args.pretrained_model_name_or_path
    tokenizer = text.load_tokenizer(name)
    text_encoder = text.load_text_encoder(name, dev, small=name.endswith("small"))
    vae = loading.load_vae(name, dev)
    unet = loading.load_unet(name, dev)
    control_lora = M.ControlLoRA.from_config(args.control_lora_config).to(dev)
    unet.set_attn_processor(M.map_processors_to_unet(unet, control_lora))
    dataset = T.build_dataset(args, tokenizer)

    logger.info("***** Running testing *****")
    logger.info("  Num examples = %d", len(dataset))
    if checkpoint is not None:
        logger.info("Resuming from checkpoint %s", os.path.basename(checkpoint))
        ControlLoRATrainer(unet, control_lora).load_state(checkpoint)   # its own layout or the reference's accelerate layout

    os.makedirs(args.output_dir, exist_ok=True)
    control_lora.save_config(args.output_dir)
    control_lora.save_pretrained(args.output_dir, safe_serialization=False)
    control_lora.save_pretrained(args.output_dir, safe_serialization=True)
    logger.info("Saved ControlLoRA to %s", args.output_dir)

    paths = sample(args, unet, control_lora, vae, text_encoder, tokenizer, dataset, dev)
    logger.info("Saved %d samples to %s", len(paths), samples_dir(args))
    return paths


if __name__ == "__main__":
    main()
