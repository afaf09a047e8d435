#!/usr/bin/env python
"""Two ControlLoRAs steering one sampler: the plain single-control sampler vs two controls on the generic path vs two controls fused.

    python tools/multi_control_bench.py --out profiles/multi_control_bench.txt
    python tools/multi_control_bench.py --version 2 --out profiles/multi_control_v2_bench.txt

* sampler: the DDIM leg of bench.py (512x512, 16 images, CFG 9.0, 50 steps, control batch 1, `random:sd15` shapes with seeded weights)
  with a second seeded v1 control model chained onto the first (models.mix_control_loras), in ONE process on one box.  The three
  arrangements are timed interleaved -- plain, generic, fused, `--reps` times over -- after a 2-step warm-up each, so that drift of
  the box lands on all three alike; the plain sampler's own run-to-run spread is the yardstick for the differences;
* launches: calls into the kernel library of one eager UNet forward (UNet batch 32) in each arrangement;
* the mix launch alone (clora_control_mix_q_f16) at the q blocks of the widest-token and the widest-channel sites:
  (32 * 4096, 320) inside a [.., 960] q|k|v output and (32 * 64, 1280) inside a [.., 3840] one, against its 4 bytes per element;
* --version 2: both models are built from configs/mpii-pose-v2.json (the decomposed form: control adds before to_q and before
  to_out); the kernel arm then times the chain launch (clora_control_chain_f16) of two rank-4 processors at (32 * 4096, 320) and
  (32 * 64, 1280) beside the four launches it replaces (a down-projection and an expand per processor), three repeats each.

Nothing is asserted: the figures are reported with the spread they were measured in."""
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
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--version", type=int, choices=(1, 2), default=1, help="control version of the two models (2: mpii-pose-v2.json)")
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

    say(f"# two ControlLoRAs in one sampler; {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    config = "fill50k.json" if a.version == 1 else "mpii-pose-v2.json"
    mix_name = "clora_control_mix_q_f16" if a.version == 1 else "clora_control_chain_f16"
    say(f"# sampler: DDIM {a.steps} steps, {a.res}x{a.res}, {a.images} images, CFG 9.0 (UNet batch {2 * a.images}), control batch 1, {config} "
        f"adapters, replayed graph; 2-step warm-up, then {a.reps} interleaved timed runs (host clock around a run that ends in a device synchronise)")
    unet, main_model = bench.build_models(dev, config=config)
    torch.manual_seed(5)
    member = M.ControlLoRA.from_config(os.path.join(ROOT, "configs", config)).to(dev)
    with torch.no_grad():
        for model, seed in ((main_model, 11), (member, 12)):     # trained models: non-zero up matrices
            g = torch.Generator(device=dev).manual_seed(seed)
            for n, q in model.named_parameters():
                if ".up.weight" in n:
                    q.normal_(0.0, 0.02, generator=g)
    batch = bench.synthetic_batch(4, a.res, dev, 42)
    g = torch.Generator(device=dev).manual_seed(1)
    nb = a.images
    cond = torch.randn(nb, 77, 768, device=dev, generator=g).half()
    uncond = torch.randn(nb, 77, 768, device=dev, generator=g).half()
    lat0 = torch.randn(nb, 4, a.res // 8, a.res // 8, device=dev, generator=g).half()
    guides = [batch["guide"][:1], batch["guide"][1:2]]

    def clear():
        for procs in main_model.lora_layers:
            for proc in procs:
                proc.pre_loras.clear(); proc.post_loras.clear()
        main_model.fold_chains(False)

    def arrange(what):
        """-> (control models, guides) of the sampler call"""
        clear()
        if what == "plain":
            unet.set_attn_processor(M.map_processors_to_unet(unet, main_model))
            return main_model, guides[0]
        M.mix_control_loras(unet, main_model, [member], pre=True, post=False, fold=what == "fused")
        return [main_model, member], guides

    def sample(what, steps):
        models, gd = arrange(what)
        return ddim_sample(unet, models, gd, cond, uncond, steps=steps, guidance_scale=9.0, latents=lat0)

    def launches(what):
        models, gd = arrange(what)
        models, gd = (models, gd) if isinstance(models, list) else ([models], [gd])
        lib = capi.lib()
        names, orig = [], lib.call
        x = torch.cat([lat0, lat0], 0)
        ehs = torch.cat([uncond, cond], 0).contiguous()
        with torch.no_grad():
            for m, g_ in reversed(list(zip(models, gd))):
                m(g_)
            unet(x, 500, ehs)
            lib.call = lambda name, *args: (names.append(name), orig(name, *args))[1]
            try:
                unet(x, 500, ehs)
            finally:
                del lib.call
            rep = main_model.fold_report()
        torch.cuda.synchronize()
        return len(names), names.count(mix_name), sum(r["folded"] for r in rep.values())

    order = ("plain", "generic", "fused")
    times, outs = {w: [] for w in order}, {}
    for w in order:
        sample(w, 2)
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for w in order:
            t = time.perf_counter()
            outs[w] = sample(w, a.steps)
            torch.cuda.synchronize()
            times[w].append(time.perf_counter() - t)
    assert all(bool(torch.isfinite(o).all()) for o in outs.values())

    def fmt(ts):
        return "  ".join(f"{t:.3f}" for t in ts) + f"  s   median {statistics.median(ts):.3f} s"

    say()
    say("## sampler latency")
    counts = {w: launches(w) for w in order}
    label = {"plain": "one control (plain sampler) ", "generic": "two controls, generic path  ", "fused": "two controls, fused sites   "}
    for w in order:
        n, nmix, nf = counts[w]
        say(f"{label[w]}: {fmt(times[w])}   library calls per UNet forward {n} ({mix_name[6:-4]} {nmix}), fused sites {nf}")
    med = {w: statistics.median(times[w]) for w in order}
    spread = (max(times["plain"]) - min(times["plain"])) / med["plain"]
    say(f"plain sampler run-to-run spread {spread * 100:.1f} %;  generic {100 * (med['generic'] / med['plain'] - 1):+.1f} % vs plain, "
        f"fused {100 * (med['fused'] / med['plain'] - 1):+.1f} % vs plain")
    gspread = max(times["generic"]) - min(times["generic"])
    say(f"generic arm's own spread {gspread * 1e3:.1f} ms; fused is {(med['generic'] - med['fused']) * 1e3:.1f} ms faster than generic (medians): "
        f"{'beats' if med['generic'] - med['fused'] > gspread else 'does NOT beat'} the generic arm by more than its spread")
    rel = lambda x, y: float((x - y).norm() / y.norm())
    say(f"latents: fused vs generic rel-L2 {rel(outs['fused'], outs['generic']):.2e}, two controls vs one {rel(outs['fused'], outs['plain']):.2e}")

    def timed(fn):
        """us per call over a.kernel_reps back-to-back calls between device events, after 5 warm-up calls"""
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.kernel_reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.kernel_reps

    if a.version == 2:
        say()
        say("## the chain launch alone (two rank-4 processors, control batch 1) beside the four launches it replaces")
        for Mr, C, rows_t in ((32 * 4096, 320, 4096), (32 * 64, 1280, 64)):
            gk = torch.Generator(device=dev).manual_seed(2)
            h = torch.randn(Mr, C, device=dev, generator=gk).half()
            y = torch.empty_like(h)
            mem = []
            for _ in range(2):
                D = torch.randn(4, C + 256, device=dev, generator=gk) / C ** 0.5
                mem.append((D, torch.randn(C, 4, device=dev, generator=gk) * 0.02, torch.randn(rows_t, 4, device=dev, generator=gk)))
            G = (torch.cat([m[0][:, :C] for m in mem], 0).double() @ torch.cat([m[1] for m in mem], 1).double()).float().contiguous()
            chain = [(D[:, :C], Uw, Tc, 0) for D, Uw, Tc in mem]
            T = torch.empty(Mr, 4, device=dev)
            h1 = torch.empty_like(h)

            def four():
                x = h
                for (D, Uw, Tc), out in zip(mem, (h1, y)):
                    K.lora_down_multi([K.down_job(x, D, T, 0, Mr, C, T_in=Tc, t_in_r=4)])
                    K.lora_up(x, T, 0, Uw, Mr, C, 0.7, out=out)
                    x = out

            four()
            ref = y.clone()
            K.control_chain(h, y, chain, G, 0.7, rows_t)
            diff = float((y.float() - ref.float()).norm() / ref.float().norm())
            t_chain = [timed(lambda: K.control_chain(h, y, chain, G, 0.7, rows_t)) for _ in range(3)]
            t_four = [timed(four) for _ in range(3)]
            f3 = lambda ts: "  ".join(f"{t:7.1f}" for t in ts)
            say(f"({Mr}, {C}): chain launch {f3(t_chain)} us (median {statistics.median(t_chain):.1f} us, "
                f"{4.0 * Mr * C / 1e9 / (statistics.median(t_chain) * 1e-6):.0f} GB/s of its 4 bytes per element);  four launches "
                f"{f3(t_four)} us (median {statistics.median(t_four):.1f} us, spread {max(t_four) - min(t_four):.1f} us);  "
                f"outputs rel-L2 {diff:.1e}")
    if a.version == 1:
        say()
        say("## the mix launch alone (one rank-4 member, control batch 1)")
        for Mr, C, rows_t in ((32 * 4096, 320, 4096), (32 * 64, 1280, 64)):
            y = torch.randn(Mr, 3 * C, device=dev).half()
            T = torch.randn(rows_t, 4, device=dev)
            Uq = torch.randn(C, 4, device=dev) * 0.02
            mem = [(T, 0, Uq, 0.49)]
            us = timed(lambda: K.control_mix_q(y, C, mem, rows_t))
            say(f"({Mr}, {C}) in a [{Mr}, {3 * C}] buffer: {us:8.1f} us per launch over {a.kernel_reps} back-to-back launches, "
                f"{4.0 * Mr * C / 1e9 / (us * 1e-6):.0f} GB/s of q-block traffic")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
