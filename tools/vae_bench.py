"""VAE encode / decode timing at SD-1.5 shapes (random weights): B images of res^2.
--attn flash|scores picks the mid-block attention path (controllora_amd.vae.VaeAttention.use_flash; above 8,192 latent tokens only
flash exists); --repeat N prints N timings of each (a path's own spread is what a difference between the paths is held against)."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from controllora_amd import vae as V, kernels as K
ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("B", type=int, nargs="?", default=4)
ap.add_argument("res", type=int, nargs="?", default=512)
ap.add_argument("--attn", choices=("flash", "scores"), default="flash" if V.VaeAttention.use_flash else "scores")
ap.add_argument("--repeat", type=int, default=1)
a = ap.parse_args()
B, res = a.B, a.res
V.VaeAttention.use_flash = a.attn == "flash"
dev = torch.device("cuda", 0)
m = V.AutoencoderKL(**V.SD15_VAE); V.init_random_(m, 1); m.to(dev)
x = (torch.rand(B, 3, res, res, device=dev) * 2 - 1).half()
def t(fn, n=3):
    fn(); torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / n * 1e3
z = m.encode(x).latent_dist.sample()
print("latent finite", bool(torch.isfinite(z).all()), float(z.abs().mean()))
img = m.decode(z.half()).sample
print("image finite", bool(torch.isfinite(img.float()).all()))
for r in range(a.repeat):
    enc = t(lambda: m.encode(x).latent_dist.sample())
    dec = t(lambda: m.decode(z.half()))
    print(f"attn={a.attn} repeat {r}: encode {enc:.2f} ms ({B} x {res}^2: {1.1167*B*(res/512)**2/enc*1e3:.0f} TFLOP/s)   decode {dec:.2f} ms ({2.5145*B*(res/512)**2/dec*1e3:.0f} TFLOP/s)")
K.PROFILER = K.KernelProfiler()
m.encode(x)
agg = K.PROFILER.summary(); K.PROFILER = None
for k, v in sorted(agg.items(), key=lambda kv: -kv[1]["ms"])[:6]:
    print(f"  {k:28s} {v['calls']:4d}x {v['ms']:8.3f} ms")
