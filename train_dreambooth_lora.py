#!/usr/bin/env python
"""DreamBooth training of a plain LoRA on the MI355X-native path: accepts the 50 flags of the reference's `parse_args`
(reference train_dreambooth_lora.py:114-384) and runs the same step (:868-920) -- VAE encode x 0.18215, noise, timesteps,
add_noise, text encode, UNet with a `LoRACrossAttnProcessor` on every attention site, fp32 MSE or, with
`--with_prior_preservation`, mse(instance) + prior_loss_weight * mse(class) over one [instance..., class...] batch, scaled
backward, clip, AdamW, LR schedule, `checkpoint-N` states -- on the gfx950 kernels (controllora_amd), one process per GPU under
`python -m torch.distributed.run`.  The result is `pytorch_lora_weights.bin` / `.safetensors` in the diffusers layout: what
`mix_lora_and_control_lora.py --lora <output_dir>` and `loading.load_lora_attn_procs` read.

    python train_dreambooth_lora.py --pretrained_model_name_or_path random:sd15 --instance_data_dir dog/ \\
        --instance_prompt "a photo of sks dog" --with_prior_preservation --class_data_dir dog_class/ \\
        --class_prompt "a photo of a dog" --max_train_steps 400 --output_dir lora-dog

What differs: `--pretrained_model_name_or_path` may be `random:sd15` / `random:small` (seeded random weights, offline); missing
class images are sampled from the frozen model with DDIM (50 steps, guidance 7.5) at `--resolution`, not with the stock
pipeline's default scheduler at 512; flags that configure services absent here (`--push_to_hub`, `--hub_*`, `--report_to`,
`--use_8bit_adam`, `--enable_xformers_memory_efficient_attention`, `--allow_tf32`, `--gradient_checkpointing`,
`--prior_generation_precision`, `--revision`) are accepted and reported as no-ops.  `--scale_lr` is applied twice, as the
reference does (:727-730 and :737-740).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import logging
import math
import os
import shutil
import time
import warnings

import torch

logger = logging.getLogger("dreambooth_lora.train")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="DreamBooth LoRA training on MI355X (reference-compatible flags).")
    p.add_argument("--pretrained_model_name_or_path", type=str, default=None, required=True)
    p.add_argument("--revision", type=str, default=None, required=False)
    p.add_argument("--tokenizer_name", type=str, default=None)
    p.add_argument("--instance_data_dir", type=str, default=None, required=True)
    p.add_argument("--class_data_dir", type=str, default=None, required=False)
    p.add_argument("--instance_prompt", type=str, default=None, required=True)
    p.add_argument("--class_prompt", type=str, default=None)
    p.add_argument("--validation_prompt", type=str, default=None)
    p.add_argument("--num_validation_images", type=int, default=4)
    p.add_argument("--validation_epochs", type=int, default=50)
    p.add_argument("--with_prior_preservation", default=False, action="store_true")
    p.add_argument("--prior_loss_weight", type=float, default=1.0)
    p.add_argument("--num_class_images", type=int, default=100)
    p.add_argument("--output_dir", type=str, default="lora-dreambooth-model")
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--resolution", type=int, default=512)
    p.add_argument("--center_crop", default=False, action="store_true")
    p.add_argument("--train_batch_size", type=int, default=4)
    p.add_argument("--sample_batch_size", type=int, default=4)
    p.add_argument("--num_train_epochs", type=int, default=1)
    p.add_argument("--max_train_steps", type=int, default=None)
    p.add_argument("--checkpointing_steps", type=int, default=500)
    p.add_argument("--checkpoints_total_limit", type=int, default=None)
    p.add_argument("--resume_from_checkpoint", type=str, default=None)
    p.add_argument("--gradient_accumulation_steps", type=int, default=1)
    p.add_argument("--gradient_checkpointing", action="store_true")
    p.add_argument("--learning_rate", type=float, default=5e-4)
    p.add_argument("--scale_lr", action="store_true", default=False)
    p.add_argument("--lr_scheduler", type=str, default="constant")
    p.add_argument("--lr_warmup_steps", type=int, default=500)
    p.add_argument("--lr_num_cycles", type=int, default=1)
    p.add_argument("--lr_power", type=float, default=1.0)
    p.add_argument("--dataloader_num_workers", type=int, default=0)
    p.add_argument("--use_8bit_adam", action="store_true")
    p.add_argument("--adam_beta1", type=float, default=0.9)
    p.add_argument("--adam_beta2", type=float, default=0.999)
    p.add_argument("--adam_weight_decay", type=float, default=1e-2)
    p.add_argument("--adam_epsilon", type=float, default=1e-08)
    p.add_argument("--max_grad_norm", default=1.0, type=float)
    p.add_argument("--push_to_hub", action="store_true")
    p.add_argument("--hub_token", type=str, default=None)
    p.add_argument("--hub_model_id", type=str, default=None)
    p.add_argument("--logging_dir", type=str, default="logs")
    p.add_argument("--allow_tf32", action="store_true")
    p.add_argument("--report_to", type=str, default="tensorboard")
    p.add_argument("--mixed_precision", type=str, default=None, choices=["no", "fp16", "bf16"])
    p.add_argument("--prior_generation_precision", type=str, default=None, choices=["no", "fp32", "fp16", "bf16"])
    p.add_argument("--local_rank", type=int, default=-1)
    p.add_argument("--enable_xformers_memory_efficient_attention", action="store_true")
    p.add_argument("--lora_rank", type=int, default=4)
    # addition (not in the reference): eager launches instead of the captured hipGraph step
    p.add_argument("--no_hipgraph", action="store_true", help="do not capture the step into hipGraphs")
    args = p.parse_args(argv)
    env_local_rank = int(os.environ.get("LOCAL_RANK", -1))
    if env_local_rank != -1 and env_local_rank != args.local_rank:
        args.local_rank = env_local_rank
    if args.with_prior_preservation:
        if args.class_data_dir is None:
            raise ValueError("You must specify a data directory for class images.")
        if args.class_prompt is None:
            raise ValueError("You must specify prompt for class images.")
    else:
        if args.class_data_dir is not None:
            warnings.warn("You need not use --class_data_dir without --with_prior_preservation.")
        if args.class_prompt is not None:
            warnings.warn("You need not use --class_prompt without --with_prior_preservation.")
    return args


def load_tokenizer(args):
    from controllora_amd import text
    if args.tokenizer_name:
        if not os.path.isdir(args.tokenizer_name):
            raise FileNotFoundError(f"--tokenizer_name {args.tokenizer_name}: not a tokenizer directory (nothing is downloaded)")
        from transformers import CLIPTokenizer
        tok = CLIPTokenizer.from_pretrained(args.tokenizer_name)
        return lambda caps: tok(list(caps), max_length=tok.model_max_length, padding="max_length", truncation=True,
                                return_tensors="pt").input_ids
    return text.load_tokenizer(args.pretrained_model_name_or_path)


def build_lora_processors(unet, rank, dev):
    """a `LoRACrossAttnProcessor` for every attention site (reference :706-722; the sizes are read off the site's own
    projections instead of the block names)"""
    from controllora_amd import models as M
    procs = {}
    for name in unet.attn_processors.keys():
        site = unet.get_submodule(name[:-len(".processor")])
        cad = None if name.endswith("attn1.processor") else unet.config.cross_attention_dim
        procs[name] = M.LoRACrossAttnProcessor(site.to_q.weight.shape[0], cad, rank=rank).to(dev)
    return procs


@torch.no_grad()
def generate_class_images(args, pipe, n_have):
    """sample the missing class images with the frozen model: `<index>-<sha1 of the pixels>.jpg` (reference :611-619)"""
    from PIL import Image
    os.makedirs(args.class_data_dir, exist_ok=True)
    res = -(-args.resolution // 64) * 64
    todo = args.num_class_images - n_have
    logger.info("Number of class images to sample: %d.", todo)
    done = 0
    while done < todo:
        n = min(args.sample_batch_size, todo - done)
        seed = None if args.seed is None else args.seed + done
        images = pipe(args.class_prompt, None, num_samples=n, ddim_steps=50, scale=7.5, seed=seed, height=res, width=res).numpy()
        for i, arr in enumerate(images):
            image = Image.fromarray(arr)
            digest = hashlib.sha1(image.tobytes()).hexdigest()
            image.save(os.path.join(args.class_data_dir, f"{done + i + n_have}-{digest}.jpg"))
        done += n


def latest_checkpoint(output_dir):
    if not os.path.isdir(output_dir):
        return None
    dirs = sorted((d for d in os.listdir(output_dir) if d.startswith("checkpoint-")), key=lambda d: int(d.split("-")[1]))
    return dirs[-1] if dirs else None


def prune_checkpoints(output_dir, limit):
    """--checkpoints_total_limit: keep the newest `limit` checkpoint directories"""
    if limit is None or limit <= 0:
        return
    dirs = sorted((d for d in os.listdir(output_dir) if d.startswith("checkpoint-")), key=lambda d: int(d.split("-")[1]))
    for d in dirs[:-limit]:
        shutil.rmtree(os.path.join(output_dir, d))


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(format="%(asctime)s - %(levelname)s - %(name)s - %(message)s", level=logging.INFO)
    from controllora_amd import data, loading, text
    from controllora_amd.pipeline import ControlLoRAPipeline
    from controllora_amd.schedulers import DDPMScheduler
    from controllora_amd.train import AttnProcsLayers, LoRATrainer

    world, rank = int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("RANK", 0))
    local = max(args.local_rank, 0)
    if not torch.cuda.is_available():
        raise RuntimeError("the DreamBooth LoRA training path needs an MI355X (no CPU fallback is provided)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        torch.distributed.init_process_group("nccl", device_id=dev)
    main_proc = rank == 0
    for flag in ("push_to_hub", "use_8bit_adam", "allow_tf32", "gradient_checkpointing", "enable_xformers_memory_efficient_attention",
                 "prior_generation_precision", "revision", "hub_token", "hub_model_id"):
        if getattr(args, flag) and main_proc:
            logger.warning("--%s is accepted for compatibility and has no effect on this path", flag)
    if args.mixed_precision == "bf16":
        logger.warning("--mixed_precision=bf16: the gfx950 kernels compute in fp16 with fp32 accumulation; using fp16")
    elif args.mixed_precision in (None, "no") and main_proc:
        logger.warning("--mixed_precision=%s: this path always computes in fp16 (fp32 accumulation, fp32 master weights) "
                       "with dynamic loss scaling; the reference would train in fp32 here", args.mixed_precision)
    if args.seed is not None:
        torch.manual_seed(args.seed + rank)            # per-rank noise / timestep / crop streams, identical model init below
    if main_proc and args.output_dir is not None:
        os.makedirs(args.output_dir, exist_ok=True)

    # ---- frozen base model (reference :644-684)
    name = args.pretrained_model_name_or_path
    tokenizer = load_tokenizer(args)
    text_encoder = text.load_text_encoder(name, dev, small=name.endswith("small"))
    vae = loading.load_vae(name, dev)
    unet = loading.load_unet(name, dev)
    noise_scheduler = DDPMScheduler()
    pipe = ControlLoRAPipeline(unet, None, vae, text_encoder, tokenizer)       # plain text-to-image on the same modules

    # ---- class images of the frozen model (reference :580-623), before any adapter is installed; rank 0 only
    if args.with_prior_preservation:
        if main_proc:
            os.makedirs(args.class_data_dir, exist_ok=True)
            have = len(os.listdir(args.class_data_dir))
            if have < args.num_class_images:
                generate_class_images(args, pipe, have)
        if world > 1:
            torch.distributed.barrier()

    # ---- trainable LoRA processors on every site (reference :706-723); seeded init from a forked stream, see the ControlLoRA script
    fork_devs = [dev.index or 0]
    with torch.random.fork_rng(devices=fork_devs):
        if args.seed is not None:
            torch.manual_seed(args.seed)
        unet.set_attn_processor(build_lora_processors(unet, args.lora_rank, dev))
    lora_layers = AttnProcsLayers(unet.attn_processors)

    for _ in range(2):                                  # the reference scales twice (:727-730, :737-740): kept
        if args.scale_lr:
            args.learning_rate = args.learning_rate * args.gradient_accumulation_steps * args.train_batch_size * world

    # ---- data (reference :765-781)
    dataset = data.DreamBoothDataset(args.instance_data_dir, args.instance_prompt, tokenizer,
                                     class_data_root=args.class_data_dir if args.with_prior_preservation else None,
                                     class_prompt=args.class_prompt, size=args.resolution, center_crop=args.center_crop)
    sampler = torch.utils.data.distributed.DistributedSampler(dataset, world, rank, shuffle=True, seed=args.seed or 0) \
        if world > 1 else None
    loader = torch.utils.data.DataLoader(dataset, shuffle=sampler is None, sampler=sampler, batch_size=args.train_batch_size,
                                         collate_fn=lambda ex: data.dreambooth_collate(ex, args.with_prior_preservation),
                                         num_workers=args.dataloader_num_workers)
    steps_per_epoch = math.ceil(len(loader) / args.gradient_accumulation_steps)
    if args.max_train_steps is None:
        args.max_train_steps = args.num_train_epochs * steps_per_epoch
    args.num_train_epochs = math.ceil(args.max_train_steps / steps_per_epoch)

    trainer = LoRATrainer(
        unet, lora_layers, lr=args.learning_rate, betas=(args.adam_beta1, args.adam_beta2), weight_decay=args.adam_weight_decay,
        eps=args.adam_epsilon, max_grad_norm=args.max_grad_norm, world_size=world,
        # fp16 kernels whatever --mixed_precision says: dynamic loss scaling is always on (see the ControlLoRA script)
        init_scale=65536.0, dynamic_scale=True, gradient_accumulation_steps=args.gradient_accumulation_steps,
        lr_lambda=data.lr_lambda(args.lr_scheduler, args.lr_warmup_steps * args.gradient_accumulation_steps,
                                 args.max_train_steps * args.gradient_accumulation_steps, power=args.lr_power,
                                 restarts=args.lr_num_cycles))

    global_step, first_epoch, resume_step = 0, 0, 0
    if args.resume_from_checkpoint:
        path = os.path.basename(args.resume_from_checkpoint) if args.resume_from_checkpoint != "latest" else latest_checkpoint(args.output_dir)
        if path is None or not os.path.isdir(os.path.join(args.output_dir, path)):
            logger.info("Checkpoint '%s' does not exist. Starting a new training run.", args.resume_from_checkpoint)
            args.resume_from_checkpoint = None
        else:
            logger.info("Resuming from checkpoint %s", path)
            trainer.load_state(os.path.join(args.output_dir, path))
            global_step = int(path.split("-")[1])
            first_epoch = global_step // steps_per_epoch
            resume_step = (global_step * args.gradient_accumulation_steps) % (steps_per_epoch * args.gradient_accumulation_steps)

    if main_proc:
        logger.info("***** Running training *****")
        logger.info("  Num examples = %d", len(dataset))
        logger.info("  Num batches each epoch = %d", len(loader))
        logger.info("  Num Epochs = %d", args.num_train_epochs)
        logger.info("  Instantaneous batch size per device = %d", args.train_batch_size)
        logger.info("  Total train batch size (w. parallel, distributed & accumulation) = %d",
                    args.train_batch_size * world * args.gradient_accumulation_steps)
        logger.info("  Gradient Accumulation steps = %d", args.gradient_accumulation_steps)
        logger.info("  Total optimization steps = %d", args.max_train_steps)

    graphed = not args.no_hipgraph and args.gradient_accumulation_steps == 1
    captured_shape = None
    # the graph's shapes are static: it is captured at the full batch only (after a resume the first batch seen may be the short
    # last one of an epoch), and batches of another size run as eager steps beside it
    full_batch = args.train_batch_size * (2 if args.with_prior_preservation else 1)
    if graphed and (len(sampler) if sampler is not None else len(dataset)) < args.train_batch_size:
        graphed = False
        if main_proc:
            logger.warning("no batch reaches --train_batch_size %d (%d examples): every step runs eagerly, no hipGraph is captured",
                           args.train_batch_size, len(dataset))
    eager_short = 0
    weights = {}                                        # UNet batch -> [1] * B/2 + [prior_loss_weight] * B/2 on the device

    def weights_for(batch):
        if not args.with_prior_preservation:
            return None
        if batch not in weights:
            weights[batch] = torch.tensor([1.0] * (batch // 2) + [args.prior_loss_weight] * (batch // 2), dtype=torch.float32, device=dev)
        return weights[batch]

    log_path = os.path.join(args.output_dir, args.logging_dir, "train_log.jsonl")
    if main_proc:
        os.makedirs(os.path.dirname(log_path), exist_ok=True)
    t_last, imgs_last = time.perf_counter(), 0

    for epoch in range(first_epoch, args.num_train_epochs):
        if sampler is not None:
            sampler.set_epoch(epoch)
        for step, batch in enumerate(loader):
            if args.resume_from_checkpoint and epoch == first_epoch and step < resume_step:
                continue
            with torch.no_grad():
                pixel = batch["pixel_values"].to(dev, non_blocking=True).half()
                latents = vae.encode(pixel).latent_dist.sample() * vae.scaling_factor
                noise = torch.randn_like(latents)
                timesteps = torch.randint(0, noise_scheduler.num_train_timesteps, (latents.shape[0],), device=dev).long()
                noisy = noise_scheduler.add_noise(latents, noise, timesteps).half()
                ehs = text_encoder(batch["input_ids"].to(dev))[0].half()
                if noise_scheduler.prediction_type == "epsilon":
                    target = noise
                elif noise_scheduler.prediction_type == "v_prediction":
                    target = noise_scheduler.get_velocity(latents, noise, timesteps)
                else:
                    raise ValueError(f"Unknown prediction type {noise_scheduler.prediction_type}")
            w = weights_for(noisy.shape[0])
            if graphed and captured_shape is None and noisy.shape[0] == full_batch:
                snap = trainer.state_dict()                 # the capture warm-up runs real steps: undo them
                trainer.capture(noisy, timesteps, ehs, target, w)
                trainer.load_state_dict(snap)
                captured_shape = tuple(noisy.shape)
            if graphed and tuple(noisy.shape) == captured_shape:
                pred = trainer.step_graphed(noisy, timesteps, ehs, target)
                stepped = True
            else:                                           # eager, or the short last batch of an epoch (the graph's shapes are static)
                if graphed:
                    eager_short += 1
                    if eager_short == 1 and main_proc:
                        logger.info("a batch of %d (the full batch is %d) runs as an eager step beside the captured one; so will "
                                    "every other short batch", noisy.shape[0], full_batch)
                pred = trainer.forward_backward(noisy, timesteps, ehs, target, w)
                stepped = trainer.optimizer_step()
            if not stepped:
                continue
            global_step += 1
            imgs_last += pixel.shape[0] * world * args.gradient_accumulation_steps
            if main_proc and (global_step % 10 == 0 or global_step == args.max_train_steps or global_step <= 3):
                now = time.perf_counter()                       # the scalars below are host syncs: only on logging steps
                rec = {"step": global_step, "epoch": epoch, "batch": int(pred.shape[0]), "step_loss": trainer.loss(pred.numel()),
                       "lr": args.learning_rate * (float(trainer.state[10]) or 1.0), "loss_scale": float(trainer.state[3]),
                       "grad_norm": float(trainer.state[9]), "images_per_s": imgs_last / (now - t_last)}
                if args.with_prior_preservation:
                    rec["instance_loss"], rec["prior_loss"] = trainer.loss_parts()
                t_last, imgs_last = now, 0
                logger.info(json.dumps(rec))
                with open(log_path, "a") as f:
                    f.write(json.dumps(rec) + "\n")
            if global_step % args.checkpointing_steps == 0 and main_proc:
                save_path = os.path.join(args.output_dir, f"checkpoint-{global_step}")
                trainer.save_state(save_path)
                prune_checkpoints(args.output_dir, args.checkpoints_total_limit)
                logger.info("Saved state to %s", save_path)
            if global_step >= args.max_train_steps:
                break
        if main_proc and args.validation_prompt is not None and epoch % args.validation_epochs == 0:
            run_validation(args, pipe, epoch)
        if global_step >= args.max_train_steps:
            break

    if world > 1:
        torch.distributed.barrier()
    if main_proc:                                           # reference :986-994: both file types
        unet.save_attn_procs(args.output_dir, weights_name=loading.LORA_WEIGHT_NAME, save_function=torch.save)
        unet.save_attn_procs(args.output_dir, weights_name=loading.LORA_WEIGHT_NAME_SAFE, safe_serialization=True)
        logger.info("Saved the LoRA to %s", args.output_dir)
    if world > 1:
        torch.distributed.destroy_process_group()
    return global_step


@torch.no_grad()
def run_validation(args, pipe, epoch):
    """sampling with the current adapters (reference :941-964): DPM-Solver++(2M), 25 steps, the pipeline's default guidance 7.5"""
    from PIL import Image
    logger.info("Running validation... Generating %d images with prompt: %s.", args.num_validation_images, args.validation_prompt)
    out_dir = os.path.join(args.output_dir, "validation")
    os.makedirs(out_dir, exist_ok=True)
    res = -(-args.resolution // 64) * 64
    for i in range(args.num_validation_images):
        img = pipe(args.validation_prompt, None, num_samples=1, ddim_steps=25, scale=7.5, seed=(args.seed or 0) + i, sampler="dpm",
                   height=res, width=res)[0].numpy()
        Image.fromarray(img).save(os.path.join(out_dir, f"epoch{epoch:04d}_{i}.png"))


if __name__ == "__main__":
    main()
