#!/usr/bin/env python
"""A frozen LoRA mixed into the ControlLoRA sampler: plain vs mixed on the generic path vs mixed and folded.

    python tools/mix_lora_bench.py --out profiles/mix_lora_fold_bench.txt

* sampler: the DDIM leg of bench.py (512x512, 16 images, CFG 9.0, 50 steps, control batch 1, the same seeded inputs and models), in ONE
  process on one box: the plain sampler, then for each arrangement (pre / post / both) the mixed sampler on the generic path
  (`fold_chain` off: what `bench.py --mix-lora` measures) and on folded weights (`ControlLoRA.fold_chains()`), each timed `--reps`
  times after a 2-step warm-up; the plain sampler is timed again at the end, so its own run-to-run spread brackets the others;
* launches: calls into the kernel library of one eager UNet forward (UNet batch 32) in each configuration;
* the fold itself: all 32 sites of SD-1.5 as one multi-job launch (clora_lora_fold_f16) against the same fold made of per-segment
  `lora_up` calls plus transposes -- host clock around a call that ends in a device synchronise, and device time between events.

The bar: the folded mixed sampler within 8 % of the plain sampler of the same run.  A miss is reported as a miss."""
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
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fold-reps", type=int, default=20)
    ap.add_argument("--arrangements", default="pre,post,both")
    ap.add_argument("--calibration", default=None, help="file holding a box calibration line to quote beside the figures")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    import bench
    from controllora_amd import capi, kernels as K, models as M
    from controllora_amd.pipeline import ddim_sample
    assert torch.cuda.is_available(), "a measurement needs the GPU (no fallback)"
    dev = torch.device("cuda")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# frozen LoRA mixed into the ControlLoRA sampler; {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    say(f"# sampler: DDIM {a.steps} steps, {a.res}x{a.res}, {a.images} images, CFG 9.0 (UNet batch {2 * a.images}), control batch 1, fill50k.json "
        f"adapters, replayed graph; 2-step warm-up, then {a.reps} timed runs (host clock around a run that ends in a device synchronise)")
    if a.calibration and os.path.exists(a.calibration):
        say("# box calibration: " + open(a.calibration).read().strip().splitlines()[-1])
    unet, clora = bench.build_models(dev)
    batch = bench.synthetic_batch(4, a.res, dev, 42)
    g = torch.Generator(device=dev).manual_seed(1)
    nb = a.images
    cond = torch.randn(nb, 77, 768, device=dev, generator=g).half()
    uncond = torch.randn(nb, 77, 768, device=dev, generator=g).half()
    lat0 = torch.randn(nb, 4, a.res // 8, a.res // 8, device=dev, generator=g).half()
    guide = batch["guide"][:1]

    def sample(steps):
        return ddim_sample(unet, clora, guide, cond, uncond, steps=steps, guidance_scale=9.0, latents=lat0)

    def timed_sampler():
        sample(2)
        torch.cuda.synchronize()
        ts, out = [], None
        for _ in range(a.reps):
            t = time.perf_counter()
            out = sample(a.steps)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        assert bool(torch.isfinite(out).all())
        return ts, out

    def launches():
        """library calls of one eager UNet forward at the sampler's batch, warm"""
        lib = capi.lib()
        names, orig = [], lib.call
        x = torch.cat([lat0, lat0], 0)
        ehs = torch.cat([uncond, cond], 0).contiguous()
        with torch.no_grad():
            clora(guide)
            unet(x, 500, ehs)
            lib.call = lambda name, *args: (names.append(name), orig(name, *args))[1]
            try:
                unet(x, 500, ehs)
            finally:
                del lib.call
        torch.cuda.synchronize()
        return len(names)

    def fmt(ts):
        return "  ".join(f"{t:.3f}" for t in ts) + f"  s   median {statistics.median(ts):.3f} s"

    def inject(arrangement):
        torch.manual_seed(11)                                   # as bench.py --mix-lora: a trained LoRA, non-zero up matrices
        for procs in clora.lora_layers:
            for proc in procs:
                other = M.LoRACrossAttnProcessor(proc.hidden_size, proc.cross_attention_dim, rank=4).to(dev)
                for q in other.parameters():
                    q.requires_grad_(False)
                    torch.nn.init.normal_(q, std=0.02)
                if arrangement in ("pre", "both"):
                    proc.inject_pre_lora(other)
                if arrangement in ("post", "both"):
                    proc.inject_post_lora(other)

    def clear():
        for procs in clora.lora_layers:
            for proc in procs:
                proc.pre_loras.clear(); proc.post_loras.clear()

    results = {}
    say()
    say("## sampler latency")
    t_plain, out_plain = timed_sampler()
    n_plain = launches()
    say(f"plain                     : {fmt(t_plain)}   launches per UNet forward {n_plain}")
    results["plain"] = t_plain
    for arr in [s for s in a.arrangements.split(",") if s]:
        inject(arr)
        clora.fold_chains(False)
        t_gen, out_gen = timed_sampler()
        n_gen = launches()
        say(f"mixed {arr:4s} generic path   : {fmt(t_gen)}   launches per UNet forward {n_gen}")
        clora.fold_chains(True)
        rep = clora.fold_report()
        assert all(r["folded"] for r in rep.values()), rep
        t_fold, out_fold = timed_sampler()
        n_fold = launches()
        d_mix = float((out_fold - out_plain).norm() / out_plain.norm())
        d_paths = float((out_fold - out_gen).norm() / out_gen.norm())
        say(f"mixed {arr:4s} folded         : {fmt(t_fold)}   launches per UNet forward {n_fold}   "
            f"(latents: folded vs generic rel-L2 {d_paths:.2e}, mixed vs plain {d_mix:.2e})")
        results[arr] = (t_gen, t_fold, n_gen, n_fold)
        clora.fold_chains(False)
        clear()
    t_plain2, _ = timed_sampler()
    say(f"plain, again at the end   : {fmt(t_plain2)}")
    allp = t_plain + t_plain2
    med_p = statistics.median(allp)
    spread = (max(allp) - min(allp)) / med_p
    say(f"plain sampler over both blocks: median {med_p:.3f} s, min {min(allp):.3f}, max {max(allp):.3f}: run-to-run spread {spread * 100:.1f} %")
    say()
    say("## the bar: folded mixed sampler within 8 % of the plain sampler of the same run")
    for arr, (t_gen, t_fold, n_gen, n_fold) in [(k, v) for k, v in results.items() if k != "plain"]:
        r_f, r_g = statistics.median(t_fold) / med_p - 1.0, statistics.median(t_gen) / med_p - 1.0
        say(f"{arr:4s}: folded {r_f * 100:+.1f} % vs plain (generic path {r_g * 100:+.1f} %) -> "
            f"{'holds' if r_f <= 0.08 else 'MISSES the bar'}"
            f"{'; inside the plain run-to-run spread' if abs(r_f) <= spread else ''}; launches folded {n_fold} = plain {n_plain}: "
            f"{'yes' if n_fold == n_plain else 'NO'}; generic {n_gen}")

    # ---- the fold itself
    say()
    say("## the fold of all sites (32 sites, 128 segments, one rank-4 member each), weights of every site rewritten in both layouts")
    inject("pre")
    clora.fold_chains(True)
    with torch.no_grad():
        assert clora.fold_now(unet, 1.0) == 32

    def timed(fn, reps):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        host, devt = [], []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t) * 1e3)
            devt.append(e0.elapsed_time(e1))
        return statistics.median(host), statistics.median(devt)

    flip = [1]                                                  # the sites are folded at scale 1.0 right now

    def refold():
        flip[0] ^= 1
        with torch.no_grad():
            n = clora.fold_now(unet, 1.0 if flip[0] else 0.5)          # another scale: every site is stale
        assert n == 32

    h_ms, d_ms = timed(refold, a.fold_reps)
    say(f"ControlLoRA.fold_now (keys, job table, upload, ONE launch)  : {h_ms:8.3f} ms host clock, {d_ms:8.3f} ms between device events")
    sites = [(m.processor, m) for m in unet.modules() if isinstance(getattr(m, "processor", None), M.LoRACrossAttnProcessor)
             and hasattr(m, "fused_packs")]
    jobs, nbytes = [], 0
    for proc, attn in sites:
        st = proc.__dict__["_fold"]
        mem = proc.pre_loras[0]
        C_ = proc.hidden_size
        for pack, segs in ((st["packs"][0], ["q"] if attn.is_cross else ["q", "k", "v"]),
                           (st["packs"][1] if attn.is_cross else None, ["k", "v"]), (st["out_pack"], ["out"])):
            if pack is None:
                continue
            for i, s in enumerate(segs):
                layer = getattr(mem, f"to_{s}_lora")
                jobs.append((pack.base.w[i * C_:(i + 1) * C_], pack.w[i * C_:(i + 1) * C_], pack.wt[:, i * C_:(i + 1) * C_],
                             layer.up.weight.detach(), layer.down.weight.detach()))
                nbytes += 3 * 2 * C_ * pack.K
    fjobs = [K.lora_fold_job(W, o, ot, [(u, d, 0.7)]) for W, o, ot, u, d in jobs]
    h1, d1 = timed(lambda: K.lora_fold_multi(fjobs), a.fold_reps)
    say(f"kernels.lora_fold_multi alone ({len(fjobs)} jobs, table upload + launch): {h1:8.3f} ms host clock, {d1:8.3f} ms between device events; "
        f"{nbytes / 1e6:.0f} MB read + written = {nbytes / 1e9 / (d1 * 1e-3):.0f} GB/s over the event interval")

    def per_segment():
        for W, o, ot, u, d in jobs:
            K.lora_up(W, u, 0, d, W.shape[0], W.shape[1], 0.7, out=o, u_tr=True)
            ot.copy_(o.t())

    h2, d2 = timed(per_segment, a.fold_reps)
    say(f"per-segment lora_up + transpose ({2 * len(jobs)} launches)            : {h2:8.3f} ms host clock, {d2:8.3f} ms between device events")
    say(f"one launch vs per-segment calls: {h2 / h1:.1f} x on the host clock, {d2 / d1:.1f} x between device events")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
