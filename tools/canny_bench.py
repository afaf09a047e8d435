#!/usr/bin/env python
"""Device Canny detector against the numpy one, and both against the train step they have to feed.

    python bench.py --gpus 1 --steps 20 --warmup 5 > bench_line.json
    python tools/canny_bench.py --bench-json bench_line.json --out profiles/canny_device_bench.txt

* device detector (`controllora_amd.kernels.canny(..., guide=True)`: classify + hysteresis groups + emit, host readbacks included),
  batch 4 and 16 at 512x512, on smoothed-noise images with thresholds drawn like the data set draws them, and on the long-snake
  worst case (hysteresis only: one weak chain of ~131,000 pixels): warm-up, then the median of `--reps` timed batches
  (host clock around a call that ends in a device synchronise), hysteresis passes and launches per batch;
* numpy detector (`controllora_amd.process.canny`) on the same images on the same machine: per image on one core, and images/s with
  `--workers` worker processes (the CPU quota of a command on the GPU machines);
* the train step (`ms_per_step` of the bench.py line given with --bench-json) and the batch-4 detector time as a share of it.

The two conditions the feature has to meet are evaluated and printed at the end; a failed one is reported as failed."""
from __future__ import annotations

import argparse
import json
import multiprocessing as mp
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def _numpy_one(job):
    from controllora_amd.process import canny
    img, lo, hi = job
    t = time.perf_counter()
    canny(img, lo, hi)
    return time.perf_counter() - t


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--numpy-images", type=int, default=32, help="images timed with the numpy detector (one core, then the pool)")
    ap.add_argument("--bench-json", default=None, help="file holding the JSON line of `bench.py --gpus 1 --steps 20 --warmup 5`")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    from controllora_amd import kernels as K
    from tests import canny_cases as CC
    assert torch.cuda.is_available(), "a measurement needs the GPU (no fallback)"
    dev, R = "cuda", a.res
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# device Canny vs numpy Canny at {R}x{R} RGB; {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    say(f"# timing: host clock around a call that ends in a device synchronise; {a.warmup} warm-up calls, median of {a.reps} timed batches")
    n_img = max(16, a.numpy_images)
    imgs = [CC.noise_image(500 + i, R, R, 3, sigma=2.0) for i in range(n_img)]
    lo, hi = CC.thresholds(77, n_img)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    device_ms = {}
    say()
    say("## device detector, smoothed-noise images (sigma 2), thresholds drawn in [1, 255) per image, guide tensor fp16 [B,3,H,W] out")
    for B in (4, 16):
        x = torch.from_numpy(np.stack(imgs[:B])).to(dev)
        tl, th = torch.from_numpy(lo[:B]).to(dev), torch.from_numpy(hi[:B]).to(dev)
        stats = {}
        K.canny(x, tl, th, guide=True, stats=stats)
        med, mn, mx = timed(lambda: K.canny(x, tl, th, guide=True))
        t_cls = timed(lambda: K.canny_classify(x, tl, th))[0]
        device_ms[B] = med
        say(f"batch {B:2d}: {med:8.3f} ms per batch (min {mn:.3f}, max {mx:.3f}) = {med / B:.3f} ms per image, {B / med * 1e3:9.0f} images/s; "
            f"hysteresis passes enqueued {stats['passes']} in {stats['groups']} group(s), launches {stats['launches']}; "
            f"classify launch alone {t_cls:.3f} ms")
    say()
    say("## device detector, long-snake worst case (hysteresis + emit on a class map with ONE weak chain of ~131,000 pixels per image)")
    for B in (4, 16):
        cls = torch.from_numpy(np.stack([CC.snake(R, R, True)] * B)).to(dev)
        stats = {}
        out = K.canny_hysteresis(cls, guide=True, stats=stats)
        assert bool((out[:, 0] > 0).eq(cls >= 1).all()), "the whole chain must light up"
        med, mn, mx = timed(lambda: K.canny_hysteresis(cls, guide=True))
        say(f"batch {B:2d}: {med:8.3f} ms per batch (min {mn:.3f}, max {mx:.3f}); hysteresis passes enqueued {stats['passes']} in "
            f"{stats['groups']} groups, launches {stats['launches']}")
    say()
    say(f"## numpy detector (controllora_amd.process.canny), the same images, this machine ({os.cpu_count()} CPUs visible, "
        f"{a.workers} allowed to a command)")
    jobs = [(imgs[i], float(lo[i]), float(hi[i])) for i in range(n_img)]
    one = [_numpy_one(j) for j in jobs[:16]]
    say(f"one core: median {statistics.median(one) * 1e3:.1f} ms per image (min {min(one) * 1e3:.1f}, max {max(one) * 1e3:.1f}) over 16 images "
        f"= {1.0 / statistics.mean(one):.1f} images/s")
    with mp.get_context("spawn").Pool(a.workers) as pool:
        pool.map(_numpy_one, jobs[:a.workers])                      # warm the workers (imports)
        many = jobs * max(1, (8 * a.workers) // n_img)
        t = time.perf_counter()
        pool.map(_numpy_one, many, chunksize=1)
        wall = time.perf_counter() - t
    pool_ips = len(many) / wall
    numpy4_ms = 4.0 / pool_ips * 1e3
    say(f"{a.workers} worker processes: {len(many)} images in {wall:.2f} s = {pool_ips:.1f} images/s, i.e. {numpy4_ms:.1f} ms for a batch of 4")
    say()
    step_ms = None
    if a.bench_json:
        for ln in open(a.bench_json):
            ln = ln.strip()
            if ln.startswith("{") and "ms_per_step" in ln:
                step_ms = float(json.loads(ln)["ms_per_step"])
    say("## against what they feed")
    if step_ms is not None:
        say(f"train step (bench.py --gpus 1 --steps 20 --warmup 5, batch 4 at 512x512, same machine, same run): {step_ms:.3f} ms per step "
            f"= {4 / step_ms * 1e3:.1f} images/s per GPU; the step's code is untouched by the detector")
        say(f"device detector, batch 4: {device_ms[4]:.3f} ms = {device_ms[4] / step_ms * 100:.2f} % of one step")
        say(f"numpy detector, batch 4 on {a.workers} cores: {numpy4_ms:.1f} ms = {numpy4_ms / step_ms * 100:.0f} % of one step; "
            f"8 GPUs need {8 * 4 / step_ms * 1e3:.0f} images/s, {a.workers} cores give {pool_ips:.0f}")
    else:
        say("train step: not measured (no --bench-json given)")
    c1 = device_ms[4] < numpy4_ms
    say(f"condition 1 (device batch of 4 cheaper than numpy for the same 4 images on all {a.workers} cores): "
        f"{device_ms[4]:.3f} ms < {numpy4_ms:.1f} ms -> {'holds' if c1 else 'FAILS'}")
    if step_ms is not None:
        c2 = device_ms[4] < step_ms
        say(f"condition 2 (device batch of 4 cheaper than one train step): {device_ms[4]:.3f} ms < {step_ms:.3f} ms -> "
            f"{'holds' if c2 else 'FAILS: the feature does not remove the bottleneck'}")
    else:
        say("condition 2: not evaluated")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
