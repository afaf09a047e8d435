#!/usr/bin/env python
"""The DreamBooth-LoRA train step and its loss launch.

    python tools/dreambooth_bench.py --out profiles/dreambooth_lora_bench.txt

* train step: `LoRATrainer` at random:sd15, 512x512 (64x64 latents), rank-4 LoRA processors on all 32 sites, replayed hipGraph
  step on seeded synthetic latents / text embeddings -- plain LoRA at batch 4, then prior preservation at batch 4 + 4 (one UNet
  pass over [instance..., class...], the per-sample-weighted loss); three timed windows of `--steps` steps each after a warm-up
  window (host clock around a window that ends in a device synchronise);
* the loss launch alone: clora_mse_weighted_f16 at (8, 16384) beside clora_mse_f16 on the same 131072 elements, `--launches`
  back-to-back launches between two device events, three repeats each, interleaved.

No target is set: the weighted launch is expected to cost what the plain one does; a difference beyond the plain launch's own
three-repeat spread is reported as such."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--base", default="random:sd15")
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rank", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    import train_dreambooth_lora as T
    from controllora_amd import kernels as K, loading
    from controllora_amd.train import AttnProcsLayers, LoRATrainer
    assert torch.cuda.is_available(), "a measurement needs the GPU (no fallback)"
    dev = torch.device("cuda")
    f16, f32 = torch.float16, torch.float32
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# DreamBooth LoRA train step and loss launch; {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    say(f"# step: {a.base}, {a.res}x{a.res}, rank-{a.rank} LoRA on every attention site, replayed hipGraph step, dynamic loss scaling; "
        f"one warm-up window, then 3 timed windows of {a.steps} steps (host clock around a window that ends in a device synchronise)")
    small = a.base.endswith("small")
    ctx = (7, 64) if small else (77, 768)
    lat = a.res // 8

    def step_bench(tag, B, prior):
        unet = loading.load_unet(a.base, dev)
        torch.manual_seed(0)
        unet.set_attn_processor(T.build_lora_processors(unet, a.rank, dev))
        tr = LoRATrainer(unet, AttnProcsLayers(unet.attn_processors), lr=5e-4)
        g = torch.Generator(device=dev).manual_seed(1)
        noisy = torch.randn(B, 4, lat, lat, device=dev, generator=g).half()
        target = torch.randn(B, 4, lat, lat, device=dev, generator=g)
        ts = torch.randint(0, 1000, (B,), device=dev, generator=g).long()
        ehs = torch.randn(B, *ctx, device=dev, generator=g).half()
        w = torch.ones(B, dtype=f32, device=dev) if prior else None        # --prior_loss_weight 1.0, the reference default
        tr.capture(noisy, ts, ehs, target, w)
        windows = []
        for i in range(4):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(a.steps):
                tr.step_graphed()
            torch.cuda.synchronize()
            if i:
                windows.append((time.perf_counter() - t) / a.steps * 1e3)
        loss = tr.loss()
        assert loss == loss and float(tr.state[6]) in (0.0, 1.0)
        med = statistics.median(windows)
        say(f"{tag:44s}: " + "  ".join(f"{x:8.2f}" for x in windows) + f"  ms/step   median {med:8.2f} ms = {B / med * 1e3:6.1f} samples/s"
            f"   (loss {loss:.4f}, loss scale {float(tr.state[3]):.0f})")
        del tr, unet
        torch.cuda.empty_cache()
        return med

    say()
    say("## train step")
    m_plain = step_bench(f"plain LoRA, batch {a.batch}", a.batch, False)
    m_prior = step_bench(f"prior preservation, batch {a.batch} + {a.batch}", 2 * a.batch, True)
    say(f"prior preservation / plain: {m_prior / m_plain:.2f} x the step time for 2 x the UNet batch")

    say()
    B, n = 8, 4 * 64 * 64
    say(f"## the loss launch alone: ({B}, {n}) = {B * n} elements, {a.launches} launches between two device events, three repeats each")
    g = torch.Generator(device=dev).manual_seed(2)
    pred = torch.randn(B, n, device=dev, generator=g).half()
    tgt = torch.randn(B, n, device=dev, generator=g).half()
    dpred = torch.empty_like(pred)
    scale = torch.tensor([65536.0], dtype=f32, device=dev)
    loss_sum, sums, ones = torch.zeros(1, dtype=f32, device=dev), torch.zeros(B, dtype=f32, device=dev), torch.ones(B, dtype=f32, device=dev)
    gs = 2.0 / (B * n)
    plain = lambda: K.mse(pred.view(-1), tgt.view(-1), loss_sum, dpred.view(-1), gs, scale)
    weighted = lambda: K.mse_weighted(pred, tgt, ones, sums, dpred, gs, scale)

    def per_launch_us(fn):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.launches * 1e3

    t_p, t_w = [], []
    for _ in range(3):
        t_p.append(per_launch_us(plain))
        t_w.append(per_launch_us(weighted))
    mp, mw = statistics.median(t_p), statistics.median(t_w)
    spread = max(t_p) - min(t_p)
    say("clora_mse_f16          : " + "  ".join(f"{x:7.2f}" for x in t_p) + f"  us/launch   median {mp:7.2f}   spread {spread:.2f}")
    say("clora_mse_weighted_f16 : " + "  ".join(f"{x:7.2f}" for x in t_w) + f"  us/launch   median {mw:7.2f}   spread {max(t_w) - min(t_w):.2f}")
    say(f"weighted - plain = {mw - mp:+.2f} us per launch: " + ("inside" if abs(mw - mp) <= spread else "OUTSIDE") +
        " the plain launch's own three-repeat spread")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
