"""The wide flash-attention forward launch (head dim 512, clora_attn_wide.hip) alone against the launches it replaces in the VAE's
mid-block attention: per image  q k^T GEMM -> clora_softmax_rows_f16 -> V^T = Wv h^T GEMM -> P V GEMM  (4 B launches; the flash path
instead projects v with one GEMM for the whole batch, timed here as `v proj`).  Device events around `--iters` calls after a warm-up,
`--repeat` windows per path, alternating; useful FLOPs = 4 B N^2 D for both paths."""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from controllora_amd import kernels as K

SHAPES = [(4, 1, 4096, 4096, 512), (1, 1, 9216, 9216, 512), (16, 1, 4096, 4096, 512)]
SCORES_MAX_TOKENS = 8192                     # clora_softmax_rows_f16 keeps a row in registers


def window(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters         # us per call


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    for B, H, N, _, D in SHAPES:
        h, q, k = ((torch.randn((B * N, D), generator=g)).half().to(dev) for _ in range(3))
        w = (torch.randn((D, D), generator=g) / math.sqrt(D)).half().to(dev)
        v = K.gemm(h, w, B * N, D, D)
        scale = 1.0 / math.sqrt(D)
        out = torch.empty_like(q)

        def flash():
            K.attn_fwd(q, k, v, B, H, N, N, D, scale, out=out)

        def vproj():
            K.gemm(h, w, B * N, D, D, out=v)

        scores = torch.empty((N, N), dtype=torch.float16, device=dev) if N <= SCORES_MAX_TOKENS else None

        def materialised():
            for b in range(B):
                qb, kb, hb = q[b * N:(b + 1) * N], k[b * N:(b + 1) * N], h[b * N:(b + 1) * N]
                K.gemm(qb, kb, N, N, D, out=scores)
                K.softmax_rows(scores, scale, out=scores)
                vt = K.gemm(w, hb, D, N, D)
                K.gemm(scores, vt, N, D, N, out=out[b * N:(b + 1) * N])

        paths = [("flash", flash), ("v proj", vproj)] + ([("scores", materialised)] if scores is not None else [])
        for _, fn in paths:
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in paths}
        for _ in range(args.repeat):
            for name, fn in paths:
                times[name].append(window(fn, args.iters))
        flops = 4.0 * B * H * N * N * D
        print(f"B={B} H={H} N={N} D={D}  useful {flops / 1e9:.1f} GFLOP")
        for name, _ in paths:
            t = times[name]
            rate = f"{flops / statistics.median(t) / 1e6:7.1f} TFLOP/s" if name != "v proj" else ""
            print(f"  {name:7s} median {statistics.median(t):10.1f} us  (min {min(t):.1f}, max {max(t):.1f})  {rate}")
        if scores is None:
            print(f"  scores  not runnable: {N} columns, clora_softmax_rows_f16 stops at {SCORES_MAX_TOKENS}")


if __name__ == "__main__":
    main()
