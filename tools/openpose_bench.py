#!/usr/bin/env python
"""OpenPose body network on the HIP kernels against its yardsticks, on one MI355X -> profiles/openpose_bench.txt.

    python tools/openpose_bench.py [--out profiles/openpose_bench.txt] [--repeats 3] [--iters 20]

Cases: the network alone at 1x184x184 (the pose app's default), 16x184x184 and 1x368x368.  Yardsticks: the same network as
torch.nn.functional.conv2d / max_pool2d in fp16 on the same GPU with the same weights (the vendor yardstick) and the fp32 torch
model on this host's CPU threads.  The three are timed interleaved, `--repeats` rounds; per round the median of `--iters` forwards
(host clock around a call that ends in a device synchronise, after 3 warm-up calls).  Also: launches per forward, and one whole
OpenposeDetector call at 512x512 with its host post-processing share.  No pass / fail threshold rides on these figures."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from controllora_amd import openpose as OP      # noqa: E402

CASES = [(1, 184, 184), (16, 184, 184), (1, 368, 368)]


class TorchNet:
    """the layer table on F.conv2d / F.max_pool2d (NCHW), the reference's concatenation order"""

    def __init__(self, sd, device, dtype):
        self.table = OP.layer_table()
        self.p = {k: v.to(device=device, dtype=dtype) for k, v in sd.items()}

    def run(self, rows, x):
        for L in rows:
            if L["ksize"] == 0:
                x = F.max_pool2d(x, 2, 2)
            else:
                x = F.conv2d(x, self.p[L["name"] + ".weight"], self.p[L["name"] + ".bias"], padding=L["ksize"] // 2)
                if L["relu"]:
                    x = F.relu(x)
        return x

    @torch.no_grad()
    def __call__(self, x):
        by = {}
        for L in self.table:
            by.setdefault(L["module"], []).append(L)
        feat = self.run(by["model0"], x)
        inp = feat
        for s in range(1, 7):
            a, b = self.run(by[f"model{s}_1"], inp), self.run(by[f"model{s}_2"], inp)
            inp = torch.cat([a, b, feat], 1)
        return a, b


def timed(fn, iters, sync):
    for _ in range(3):
        fn()
    sync()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles", "openpose_bench.txt"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu_iters", type=int, default=2)
    a = ap.parse_args(argv)
    dev = "cuda"
    sd = OP.random_state_dict(0)
    net = OP.BodyPoseNet(sd, dev)
    vendor = TorchNet(sd, dev, torch.float16)
    host = TorchNet(sd, "cpu", torch.float32)
    lines = [f"# OpenPose body network (92 convolutions, 3 pools), random:openpose weights; {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             f"# timing: host clock around a forward that ends in a device synchronise; 3 warm-up calls, median of {a.iters} forwards per round, "
             f"{a.repeats} interleaved rounds (HIP kernels, torch fp16 on the same GPU, torch fp32 on {torch.get_num_threads()} CPU threads)", ""]
    for B, H, W in CASES:
        g = torch.Generator().manual_seed(1)
        x = (torch.rand(B, 3, H, W, generator=g) - 0.5)
        xd = x.half().to(dev)
        ours, theirs, cpu = [], [], []
        for _ in range(a.repeats):
            ours.append(timed(lambda: net(xd), a.iters, torch.cuda.synchronize))
            theirs.append(timed(lambda: vendor(xd), a.iters, torch.cuda.synchronize))
            if B == 1:
                cpu.append(timed(lambda: host(x), a.cpu_iters, lambda: None))
        p, h = net(xd)
        vp, vh = vendor(xd)
        rel = float((p.float() - vp.float()).norm() / vp.float().norm()), float((h.float() - vh.float()).norm() / vh.float().norm())
        fmt = lambda v: " ".join(f"{t:9.3f}" for t in v)
        lines += [f"## {B}x3x{H}x{W}: {net.launches} launches per forward; rel-L2 against torch fp16: paf {rel[0]:.2e}, heat {rel[1]:.2e}",
                  f"HIP kernels       ms per forward, per round: {fmt(ours)}   median {statistics.median(ours):9.3f}",
                  f"torch fp16 (GPU)  ms per forward, per round: {fmt(theirs)}   median {statistics.median(theirs):9.3f}   "
                  f"= {statistics.median(theirs) / statistics.median(ours):.2f} x the HIP kernels' time"]
        if cpu:
            lines.append(f"torch fp32 (CPU)  ms per forward, per round: {fmt(cpu)}   median {statistics.median(cpu):9.3f}")
        lines.append("")
    photo = np.random.default_rng(0).integers(0, 256, (512, 512, 3), dtype=np.uint8)
    det = OP.OpenposeDetector("random:openpose", dev)
    det(photo)
    rows = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        _, pose = det(photo)
        total = (time.perf_counter() - t0) * 1e3
        tm = det.body_estimation.timings
        rows.append((total, tm["maps_s"] * 1e3, tm["postprocess_s"] * 1e3, len(pose["candidate"])))
    lines.append("## one OpenposeDetector call on a 512x512 noise photo (random weights: the peak count is that of noise, not of a person)")
    for total, maps, post, n in rows:
        lines.append(f"total {total:9.1f} ms: resize + network + map resize {maps:9.1f} ms, host post-processing {post:9.1f} ms "
                     f"({100 * post / total:.0f} %), drawing {total - maps - post:7.1f} ms; {n} candidates")
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
