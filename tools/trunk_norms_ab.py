"""A/B of CLORA_TRUNK_LO=infer against CLORA_TRUNK_LO=norms (the GroupNorm / LayerNorm forwards of trunk tensors read hi + lo):
one process, one GPU, the two modes interleaved, three repeats.

    python tools/trunk_norms_ab.py [--repeats 3] [--out profiles/trunk_norms_ab.txt]

Per mode and repeat:
  - the batch-32 first evaluation and the latents after scheduler steps 1 and 5 against tests/golden/full_infer_512_b32.safetensors,
  - the DDIM-50 latents against tests/golden/full_ddim_512_50.safetensors,
  - DDIM-50 wall time for 16 images at 512x512 (UNet batch 32, `pipeline.ddim_sample` as shipped: warm-up forward, capture, 50 replays;
    a host clock around work that ends in a device synchronise) and the peak device memory of that call,
and once per mode the C-ABI calls of one eager UNet forward at batch 32 (counted at the binding, after a warm-up forward).
The mode is switched through kernels.TRUNK_LO_MODE, which is what the environment variable sets."""
from __future__ import annotations

import argparse
import collections
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("infer", "norms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("trunk_norms_ab.py measures on a GPU; none is visible")
    from controllora_amd import capi
    from controllora_amd import kernels as K
    from controllora_amd.pipeline import ddim_sample
    from oracle.make_fullsize_golden import infer32_inputs
    from tests import full_cases as FC
    dev = "cuda"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/trunk_norms_ab.py  repeats={a.repeats}  device={torch.cuda.get_device_name(0)}  "
        f"build={capi.lib().cdll.clora_build_info().decode()}")
    fx, meta = FC.load_fixture("full_infer_512_b32.safetensors")
    _, _, p_unet, p_clora = FC.build_pair(meta["config"], dev)
    guide, cond, uncond, lat0 = (t.to(dev).half() for t in infer32_inputs(int(meta["res"]), int(meta["images"]), int(meta["input_seed"])))
    steps, scale = int(meta["steps"]), float(meta["guidance_scale"])
    say(f"# sampler workload: {lat0.shape[0]} images at {int(meta['res'])}^2, UNet batch {2 * lat0.shape[0]}, {steps} DDIM steps, CFG {scale}")

    def sample():
        return ddim_sample(p_unet, p_clora, guide, cond, uncond, steps=steps, guidance_scale=scale, latents=lat0.clone(), graph=True)

    # ---- library calls of one eager forward at batch 32
    x_in = torch.cat([lat0, lat0], 0)
    ehs = torch.cat([uncond, cond], 0).contiguous()
    calls = {}
    with torch.no_grad():
        p_clora(guide)
        for mode in MODES:
            K.TRUNK_LO_MODE = mode
            p_unet(x_in, 801, ehs)                                    # lazy packs, allocator
            cnt = collections.Counter()
            orig = capi.Lib.call

            def counting(lib, name, *args, _cnt=cnt, _orig=orig):
                _cnt[name] += 1
                return _orig(lib, name, *args)
            capi.Lib.call = counting
            try:
                p_unet(x_in, 801, ehs)
            finally:
                capi.Lib.call = orig
            torch.cuda.synchronize()
            calls[mode] = cnt
    say("\n## C-ABI calls of one eager UNet forward at batch 32 (a split-K GEMM call or a two-launch GroupNorm call is more than one kernel)")
    names = sorted(set(calls["infer"]) | set(calls["norms"]))
    say(f"{'entry point':38s} {'infer':>7s} {'norms':>7s}")
    for n in names:
        say(f"{n:38s} {calls['infer'][n]:7d} {calls['norms'][n]:7d}")
    say(f"{'total':38s} {sum(calls['infer'].values()):7d} {sum(calls['norms'].values()):7d}")

    # ---- accuracy, wall time, peak memory: interleaved
    for mode in MODES:                                                # one untimed sampling run per mode
        K.TRUNK_LO_MODE = mode
        sample()
    torch.cuda.synchronize()
    rec = {m: collections.defaultdict(list) for m in MODES}
    for r in range(a.repeats):
        for mode in MODES:
            K.TRUNK_LO_MODE = mode
            e32 = FC.infer32_vs_fixture(dev)
            edd = FC.ddim_vs_fixture(dev)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            out = sample()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert torch.isfinite(out).all()
            peak = torch.cuda.max_memory_allocated()
            d = rec[mode]
            d["b32_eps_step01"].append(e32["eps_step01"]); d["b32_eps_worst_sample"].append(e32["eps_step01_worst_sample"])
            d["b32_latents_step01"].append(e32.get("latents_step01", float("nan"))); d["b32_latents_step05"].append(e32.get("latents_step05", float("nan")))
            d["ddim50_eps_step01"].append(edd["eps_step01"]); d["ddim50_latents"].append(edd["latents"])
            d["wall_s"].append(dt); d["peak_MiB"].append(peak / 2**20); d["peak_over_start_MiB"].append((peak - base) / 2**20)
            say(f"repeat {r} {mode:5s}: b32 eps {e32['eps_step01']:.4e} (worst sample {e32['eps_step01_worst_sample']:.4e}) "
                f"latents step1 {d['b32_latents_step01'][-1]:.4e} step5 {d['b32_latents_step05'][-1]:.4e} | DDIM-50 eps {edd['eps_step01']:.4e} "
                f"latents {edd['latents']:.4e} | 16 images DDIM-50 wall {dt:.4f} s peak {peak / 2**20:.0f} MiB")
    K.TRUNK_LO_MODE = os.environ.get("CLORA_TRUNK_LO", "infer")
    assert K.gn_team_errors(dev) == 0

    say("\n## summary (median of the repeats; errors are rel-L2 against the fp32 oracle fixtures, contract 1e-3)")
    say(f"{'figure':28s} {'infer':>12s} {'norms':>12s}")
    for k in ("b32_eps_step01", "b32_eps_worst_sample", "b32_latents_step01", "b32_latents_step05", "ddim50_eps_step01", "ddim50_latents"):
        say(f"{k:28s} {statistics.median(rec['infer'][k]):12.4e} {statistics.median(rec['norms'][k]):12.4e}")
    for k in ("wall_s", "peak_MiB", "peak_over_start_MiB"):
        say(f"{k:28s} {statistics.median(rec['infer'][k]):12.4f} {statistics.median(rec['norms'][k]):12.4f}")
    wi, wn = rec["infer"]["wall_s"], rec["norms"]["wall_s"]
    spread = (max(wi) - min(wi)) / statistics.median(wi) * 100
    delta = (statistics.median(wn) - statistics.median(wi)) / statistics.median(wi) * 100
    say(f"wall time: infer {' '.join(f'{v:.4f}' for v in wi)} s (spread {spread:.2f} % of its median); norms {' '.join(f'{v:.4f}' for v in wn)} s; "
        f"norms - infer = {delta:+.2f} % of infer's median")
    say(f"peak memory of the sampling call: norms - infer = {statistics.median(rec['norms']['peak_MiB']) - statistics.median(rec['infer']['peak_MiB']):+.0f} MiB")
    for k in ("ddim50_latents", "b32_eps_step01"):
        say(f"distance to 1e-3, {k}: infer {statistics.median(rec['infer'][k]) - 1e-3:+.3e}  norms {statistics.median(rec['norms'][k]) - 1e-3:+.3e}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
