#!/usr/bin/env python
"""Several ControlLoRAs steering one image (canny + pose): the reference chains further control processors onto the main model's
with `inject_pre_lora` (reference models.py:232-243); here the chained members are frozen and every site runs fused
(controllora_amd.models.mix_control_loras).  Command-line form in the style of apps/canny2image.py:

    python apps/multi_control2image.py --base /path/to/stable-diffusion-v1-5 \\
        --control_lora /path/to/canny-control-lora --guide canny \\
        --control_lora /path/to/pose-control-lora --guide pose_map.png \\
        --input photo.png --prompt "a dancer" --out out.png

`--control_lora DIR` and `--guide PATH` come in pairs, the main model first.  `--guide canny` makes that guide from `--input` with the
canny app's detector options, `--guide openpose` runs the OpenPose body detector (`--openpose PATH|random:openpose`) on it as the pose
app does; any other value is an image file used as it is (resized to the generated size).  The output is
[guide_0 | guide_1 | ... | images].  `--no_fold` keeps the chained members on the unfused path.
"""
from __future__ import annotations

import argparse
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))

from canny2image import detect, hwc3, resize_image          # noqa: E402


def load_guides(specs, input_image, image_resolution, low, high, detector, openpose=None, detect_resolution=512):
    """-> (uint8 [H,W,3] maps as shown in the output strip, float control tensors [1,3,H,W] in [-1, 1]), all of one size"""
    import torch
    from PIL import Image
    base = resize_image(hwc3(input_image), image_resolution) if input_image is not None else None
    shown, controls = [], []
    size = None if base is None else base.shape[:2]
    for spec in specs:
        if spec == "canny":
            if base is None:
                raise SystemExit("--guide canny needs --input")
            detected = hwc3(detect(base, low, high, detector))
            shown.append(255 - detected)
        elif spec == "openpose":
            if input_image is None or openpose is None:
                raise SystemExit("--guide openpose needs --input and --openpose")
            from pose2image import nearest_resize
            pose_map, _ = openpose(resize_image(hwc3(input_image), detect_resolution))       # reference apps/gradio_pose2image.py:75-77
            detected = nearest_resize(hwc3(pose_map), base.shape[1], base.shape[0])
            shown.append(detected)
        else:
            img = hwc3(np.asarray(Image.open(spec).convert("RGB")))
            if size is None:
                size = resize_image(img, image_resolution).shape[:2]
            detected = np.asarray(Image.fromarray(img).resize((size[1], size[0]), Image.BOX))
            shown.append(detected)
        controls.append(torch.from_numpy(detected[..., ::-1].copy().transpose(2, 0, 1)).float()[None] / 127.5 - 1.0)
    return shown, controls


def process(pipe, guides_shown, controls, prompt, a_prompt, n_prompt, num_samples, sample_steps, scale, seed, sampler="dpm", sampler_step="host"):
    if seed == -1:
        seed = random.randint(0, 65535)
    images = pipe(prompt, controls, a_prompt=a_prompt, n_prompt=n_prompt, num_samples=num_samples, ddim_steps=sample_steps,
                  scale=scale, seed=seed, sampler=sampler, step_impl=sampler_step)
    return list(guides_shown) + [im.numpy() for im in images]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--base", required=True, help="SD-1.5 checkpoint directory (diffusers layout) or random:sd15 / random:sd15-small")
    ap.add_argument("--control_lora", action="append", required=True, help="directory written by ControlLoRA.save_pretrained; repeat, main model first")
    ap.add_argument("--guide", action="append", required=True, help="'canny' or 'openpose' (made from --input) or an image file; one per --control_lora, same order")
    ap.add_argument("--input", default=None, help="the image `--guide canny` / `--guide openpose` read")
    ap.add_argument("--openpose", default=None, metavar="PATH|random:openpose", help="body_pose_model.pth for `--guide openpose`")
    ap.add_argument("--detect_resolution", type=int, default=512, help="short side of the OpenPose detector's input")
    ap.add_argument("--prompt", required=True)
    ap.add_argument("--a_prompt", default="best quality, extremely detailed")
    ap.add_argument("--n_prompt", default="longbody, lowres, bad anatomy, bad hands, missing fingers, extra digit, fewer digits, cropped, worst quality, low quality")
    ap.add_argument("--num_samples", type=int, default=1)
    ap.add_argument("--image_resolution", type=int, default=512,
                    help="short side of the generated image; both sides become multiples of 64")
    ap.add_argument("--sample_steps", type=int, default=20)
    ap.add_argument("--scale", type=float, default=9.0)
    ap.add_argument("--seed", type=int, default=-1)
    ap.add_argument("--low_threshold", type=int, default=100)
    ap.add_argument("--high_threshold", type=int, default=200)
    ap.add_argument("--sampler", default="dpm", choices=["dpm", "ddim"])
    ap.add_argument("--sampler_step", default="host", choices=["host", "device"],
                    help="scheduler step as torch ops on the latents (host) or as one HIP launch per step (device)")
    ap.add_argument("--detector", default="numpy", choices=["numpy", "device"], help="Canny on the CPU (numpy) or on the GPU (HIP kernels)")
    ap.add_argument("--no_fold", action="store_true", help="keep the chained control models on the unfused path")
    ap.add_argument("--out", default="multi_control2image.png")
    a = ap.parse_args(argv)
    if len(a.control_lora) != len(a.guide):
        raise SystemExit(f"{len(a.control_lora)} --control_lora and {len(a.guide)} --guide: they come in pairs")
    import torch
    from PIL import Image
    from controllora_amd.pipeline import ControlLoRAPipeline
    pipe = ControlLoRAPipeline.from_pretrained(a.base, list(a.control_lora), fold=not a.no_fold)
    inp = np.asarray(Image.open(a.input).convert("RGB")) if a.input else None
    openpose = None
    if "openpose" in a.guide:
        if not a.openpose:
            raise SystemExit("--guide openpose needs --openpose PATH|random:openpose")
        from controllora_amd.openpose import OpenposeDetector
        openpose = OpenposeDetector(a.openpose)
    shown, controls = load_guides(a.guide, inp, a.image_resolution, a.low_threshold, a.high_threshold, a.detector, openpose, a.detect_resolution)
    results = process(pipe, shown, controls, a.prompt, a.a_prompt, a.n_prompt, a.num_samples, a.sample_steps, a.scale, a.seed, a.sampler,
                      a.sampler_step)
    with torch.no_grad():
        rep = pipe.control_lora[0].fold_report()
    fused = sum(r["folded"] for r in rep.values())
    print(f"{len(a.control_lora)} control models, {fused} of {len(rep)} sites fused")
    for why in sorted({r["reason"] for r in rep.values() if r["reason"]}):
        print("  not fused:", why)
    Image.fromarray(np.concatenate(results, axis=1)).save(a.out)
    print("wrote", a.out)
    return fused


if __name__ == "__main__":
    main()
