"""Frozen base-model loading for the entry points: a checkpoint directory in the diffusers SD-1.5 layout
(`unet/`, `vae/`, `text_encoder/`, `tokenizer/` with `diffusion_pytorch_model.{safetensors,bin}`), as the reference
loads at train_text_to_image_control_lora.py:395-409, or -- because no weights are reachable offline -- the
pseudo-names `random:sd15` / `random:small` = seeded random weights at the SD-1.5 (or the tests' small) shapes."""
from __future__ import annotations

import json
import os

import torch

from . import unet as U
from . import vae as V

# newer diffusers releases renamed the VAE attention keys; accept both spellings
_VAE_RENAMES = {".to_q.": ".query.", ".to_k.": ".key.", ".to_v.": ".value.", ".to_out.0.": ".proj_attn."}

SMALL_UNET = dict(in_channels=4, out_channels=4, block_out_channels=(32, 64, 128, 128), layers_per_block=2,
                  attention_head_dim=4, cross_attention_dim=64, norm_num_groups=8, norm_eps=1e-5)
SMALL_VAE = dict(in_channels=3, out_channels=3, latent_channels=4, block_out_channels=(16, 32, 32, 64),
                 layers_per_block=1, norm_num_groups=8)


def _read_state_dict(folder: str):
    safe, pt = os.path.join(folder, "diffusion_pytorch_model.safetensors"), os.path.join(folder, "diffusion_pytorch_model.bin")
    if os.path.exists(safe):
        from safetensors.torch import load_file
        return load_file(safe)
    if os.path.exists(pt):
        return torch.load(pt, map_location="cpu", weights_only=True)
    raise FileNotFoundError(f"no diffusion_pytorch_model.safetensors / .bin under {folder}")


def _load_into(module, sd, renames=None):
    own = module.state_dict()
    if renames:
        sd = {_rename(k, renames): v for k, v in sd.items()}
    missing, extra = sorted(set(own) - set(sd)), sorted(set(sd) - set(own))
    if missing or extra:
        raise ValueError(f"checkpoint does not match the model: missing {missing[:4]} unexpected {extra[:4]}")
    with torch.no_grad():
        for k, v in own.items():
            v.copy_(sd[k].reshape(v.shape).to(v.dtype))


def _rename(k, renames):
    for a, b in renames.items():
        k = k.replace(a, b)
    return k


def is_random(name: str) -> bool:
    return name.startswith("random:")


def load_unet(name: str, device, seed: int = 0) -> U.UNet2DConditionModel:
    if is_random(name):
        unet = U.UNet2DConditionModel(**(SMALL_UNET if name.endswith("small") else {}))
        unet.to(device)
        U.init_random_(unet, seed=seed)
        return unet
    folder = os.path.join(name, "unet")
    cfg = json.load(open(os.path.join(folder, "config.json")))
    keep = ("in_channels", "out_channels", "block_out_channels", "layers_per_block", "down_block_types", "up_block_types",
            "attention_head_dim", "cross_attention_dim", "norm_num_groups", "norm_eps")
    unet = U.UNet2DConditionModel(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in cfg.items() if k in keep})
    _load_into(unet, {k: v for k, v in _read_state_dict(folder).items()})
    return unet.to(device)


def load_vae(name: str, device, seed: int = 1) -> V.AutoencoderKL:
    if is_random(name):
        vae = V.AutoencoderKL(**(SMALL_VAE if name.endswith("small") else V.SD15_VAE))
        V.init_random_(vae, seed=seed)
        return vae.to(device)
    folder = os.path.join(name, "vae")
    cfg = json.load(open(os.path.join(folder, "config.json")))
    keep = ("in_channels", "out_channels", "latent_channels", "block_out_channels", "layers_per_block", "norm_num_groups",
            "scaling_factor")
    vae = V.AutoencoderKL(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in cfg.items() if k in keep})
    _load_into(vae, _read_state_dict(folder), _VAE_RENAMES)
    return vae.to(device)


# ---- plain LoRA files in the diffusers layout (`AttnProcsLayers(unet.attn_processors)` / `save_attn_procs`): what the reference's
# train_dreambooth_lora.py saves and its mix_lora_and_control_lora.py:124-130 loads on top of the ControlLoRA processors
LORA_FILE_NAMES = ("pytorch_lora_weights.safetensors", "pytorch_lora_weights.bin", "diffusion_pytorch_model.safetensors",
                   "diffusion_pytorch_model.bin")
_LORA_PARTS = tuple(f"to_{p}_lora.{d}.weight" for p in ("q", "k", "v", "out") for d in ("down", "up"))


def _read_lora_file(path: str):
    if os.path.isdir(path):
        hit = next((os.path.join(path, n) for n in LORA_FILE_NAMES if os.path.exists(os.path.join(path, n))), None)
        if hit is None:
            raise FileNotFoundError(f"none of {', '.join(LORA_FILE_NAMES)} under {path}")
        path = hit
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    return torch.load(path, map_location="cpu", weights_only=True)


def load_lora_attn_procs(unet, path_or_state_dict) -> dict:
    """-> {attention processor name of `unet`: models.LoRACrossAttnProcessor} carrying the weights of a diffusers-format LoRA:
    keys `<attention module path>.processor.to_{q,k,v,out}_lora.{down,up}.weight`; rank and sizes are read off the tensor
    shapes.  Accepts a state dict, a `.bin` / `.safetensors` file or a folder holding one of LORA_FILE_NAMES.  The processors
    are created on the UNet's device, in fp32, frozen or not as the caller decides (they come back trainable, like any module)."""
    from . import models
    sd = path_or_state_dict if isinstance(path_or_state_dict, dict) else _read_lora_file(str(path_or_state_dict))
    names = list(unet.attn_processors.keys())
    want = {f"{n}.{part}" for n in names for part in _LORA_PARTS}
    missing, extra = sorted(want - set(sd)), sorted(set(sd) - want)
    if missing or extra:
        raise ValueError(f"LoRA file does not match the UNet's attention sites: missing {missing[:4]} unexpected {extra[:4]}")
    dev = next(unet.parameters()).device
    procs = {}
    for n in names:
        site = unet.get_submodule(n[:-len(".processor")])
        q_down, k_down = sd[f"{n}.to_q_lora.down.weight"], sd[f"{n}.to_k_lora.down.weight"]
        rank, hidden = q_down.shape
        cad = k_down.shape[1] if getattr(site, "is_cross", n.endswith("attn2.processor")) else None
        proc = models.LoRACrossAttnProcessor(hidden, cad, rank=rank)
        _load_into(proc, {part: sd[f"{n}.{part}"] for part in _LORA_PARTS})
        procs[n] = proc.to(dev)
    return procs


LORA_WEIGHT_NAME, LORA_WEIGHT_NAME_SAFE = "pytorch_lora_weights.bin", "pytorch_lora_weights.safetensors"


def lora_state_dict(unet_or_procs) -> dict:
    """{`<site>.processor.to_{q,k,v,out}_lora.{down,up}.weight`: fp32 CPU tensor} of plain LoRA processors: a UNet (its
    `attn_processors`), a {processor name: processor} dict or a `train.AttnProcsLayers`"""
    from . import models
    if hasattr(unet_or_procs, "attn_processors"):
        procs = unet_or_procs.attn_processors
    elif hasattr(unet_or_procs, "named_processors"):
        procs = unet_or_procs.named_processors()
    else:
        procs = dict(unet_or_procs)
    sd = {}
    for n, proc in procs.items():
        if type(proc) is not models.LoRACrossAttnProcessor or proc.post_add:
            raise ValueError(f"{n}: {type(proc).__name__} is not a plain LoRA processor; the diffusers LoRA file holds nothing else")
        own = proc.state_dict()
        miss = [part for part in _LORA_PARTS if part not in own]
        if miss:
            raise ValueError(f"{n}: the processor has no {miss[0]} (a skipped segment cannot be written to a LoRA file)")
        for part in _LORA_PARTS:
            sd[f"{n}.{part}"] = own[part].detach().to("cpu", torch.float32).contiguous().clone()
    return sd


def save_lora_attn_procs(unet_or_procs, directory: str, weights_name: str = None, safe_serialization: bool = False) -> str:
    """Write the file `load_lora_attn_procs` reads (what the reference's `unet.save_attn_procs` writes,
    train_dreambooth_lora.py:986-994): `pytorch_lora_weights.bin` (torch.save) or `.safetensors`.  -> the path written"""
    sd = lora_state_dict(unet_or_procs)
    os.makedirs(directory, exist_ok=True)
    if weights_name is None:
        weights_name = LORA_WEIGHT_NAME_SAFE if safe_serialization else LORA_WEIGHT_NAME
    path = os.path.join(directory, weights_name)
    if safe_serialization or weights_name.endswith(".safetensors"):
        from safetensors.torch import save_file
        save_file(sd, path)
    else:
        torch.save(sd, path)
    return path
