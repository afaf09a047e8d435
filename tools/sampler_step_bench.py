#!/usr/bin/env python
"""The scheduler step between two UNet replays: torch ops on the latents (`step_impl="host"`) against the one-launch sampler step
(`step_impl="device"`, clora_sampler_step_f16), in ONE process on one box.

    python tools/sampler_step_bench.py --out profiles/sampler_step_bench.txt

Three configurations on `random:sd15` shapes with seeded weights and the fill50k adapters, replayed graph, control batch 1:
* DDIM 50 steps for 16 images at 512 x 512, CFG 9.0 (the README's sampler figure);
* DPM-Solver++(2M) 20 steps for 1 image at 512 x 512 (the apps' default);
* DDIM 50 steps for 16 images with eta = 1 (one noise tensor per step, given up front).
For each: wall time of `--reps` interleaved runs of both paths after a 2-step warm-up each (host clock around a run that ends in
a device synchronise; the run includes the graph capture, as bench.py's DDIM leg does); the GPU work enqueued per step OUTSIDE
the replayed graph, from a torch.profiler pass of its own -- runtime launch / copy / fill calls of a 16-step run minus those of
an 8-step run, over 8 (what both runs do once cancels; a graph replay is one call of its own and is listed beside them); and the
rel-L2 of the final latents between the two paths (fp32 summation order, amplified through the fp16 UNet input).

Nothing is asserted: the figures are reported with the spread they were measured in."""
from __future__ import annotations

import argparse
import collections
import os
import re
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

ENQUEUE = re.compile(r"^hip(Ext)?(Module)?Launch(Cooperative)?Kernel|^hipLaunchByPtr|^hipMemcpy|^hipMemset")
REPLAY = re.compile(r"^hipGraphLaunch")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None, help="run one configuration: ddim50, dpm20 or ddim50_eta1")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    import bench
    from controllora_amd.pipeline import ddim_sample
    assert torch.cuda.is_available(), "a measurement needs the GPU (no fallback)"
    dev = torch.device("cuda")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# scheduler step between UNet replays: host torch ops vs one launch; {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    say(f"# {a.res}x{a.res}, random:sd15 shapes, fill50k.json adapters, control batch 1, replayed graph; 2-step warm-up of each path, then "
        f"{a.reps} interleaved timed runs (host clock around a run that ends in a device synchronise, graph capture included)")
    unet, clora = bench.build_models(dev)
    batch = bench.synthetic_batch(4, a.res, dev, 42)
    guide = batch["guide"][:1]
    configs = {"ddim50": dict(images=16, sampler="ddim", steps=50, scale=9.0, eta=0.0),
               "dpm20": dict(images=1, sampler="dpm", steps=20, scale=9.0, eta=0.0),
               "ddim50_eta1": dict(images=16, sampler="ddim", steps=50, scale=9.0, eta=1.0)}
    label = {"ddim50": "DDIM 50 steps, 16 images", "dpm20": "DPM-Solver++(2M) 20 steps, 1 image", "ddim50_eta1": "DDIM 50 steps, 16 images, eta = 1"}
    impls = ("host", "device")

    for name, cfg in configs.items():
        if a.only and name != a.only:
            continue
        g = torch.Generator(device=dev).manual_seed(1)
        nb, side = cfg["images"], a.res // 8
        cond = torch.randn(nb, 77, 768, device=dev, generator=g).half()
        uncond = torch.randn(nb, 77, 768, device=dev, generator=g).half()
        lat0 = torch.randn(nb, 4, side, side, device=dev, generator=g).half()

        def sample(impl, steps):
            noise = None
            if cfg["eta"]:
                noise = torch.randn(steps, nb, 4, side, side, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
            return ddim_sample(unet, clora, guide, cond, uncond, steps=steps, guidance_scale=cfg["scale"], latents=lat0, sampler=cfg["sampler"],
                               eta=cfg["eta"], noise=noise, graph=True, step_impl=impl)

        def enqueued(impl, steps):
            """-> Counter of runtime calls that enqueue GPU work during one run"""
            from torch.profiler import ProfilerActivity, profile
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                sample(impl, steps)
                torch.cuda.synchronize()
            return collections.Counter(e.name for e in prof.events() if e.name.startswith("hip"))

        times, outs = {w: [] for w in impls}, {}
        for w in impls:
            sample(w, 2)
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for w in impls:
                t = time.perf_counter()
                outs[w] = sample(w, cfg["steps"])
                torch.cuda.synchronize()
                times[w].append(time.perf_counter() - t)
        assert all(bool(torch.isfinite(o).all()) for o in outs.values())
        say()
        say(f"## {label[name]}")
        per_step = {}
        for w in impls:
            short, long_ = enqueued(w, 8), enqueued(w, 16)
            diff = {k: (long_[k] - short[k]) / 8.0 for k in set(long_) | set(short) if long_[k] != short[k]}
            per_step[w] = (sum(v for k, v in diff.items() if ENQUEUE.match(k)), sum(v for k, v in diff.items() if REPLAY.match(k)), diff)
        for w in impls:
            ts = times[w]
            n, r, diff = per_step[w]
            say(f"{w:6s}: " + "  ".join(f"{t:.3f}" for t in ts) + f"  s   median {statistics.median(ts):.3f} s   spread {(max(ts) - min(ts)) * 1e3:.1f} ms   "
                f"enqueued per step outside the graph: {n:.2f} launches / copies / fills (+ {r:.2f} graph replay)")
            say("        per step by runtime call: " + ", ".join(f"{k} {v:.2f}" for k, v in sorted(diff.items())))
        mh, md = statistics.median(times["host"]), statistics.median(times["device"])
        spread = max(times["host"]) - min(times["host"])
        say(f"device vs host (medians): {(md - mh) * 1e3:+.1f} ms ({100 * (md / mh - 1):+.2f} %), {(md - mh) * 1e3 / cfg['steps']:+.3f} ms per step; host's own "
            f"{a.reps}-repeat spread {spread * 1e3:.1f} ms: device is {'NOT slower' if md - mh <= spread else 'SLOWER'} than host by more than that spread")
        say(f"final latents, device vs host: rel-L2 {float((outs['device'] - outs['host']).norm() / outs['host'].norm()):.3e}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
