"""Shared inputs and the numpy restatement for the device Canny tests (tests/test_canny_emu.py, tests/test_canny_gpu.py).

`classify_np` + `hysteresis_np` are the lines of `controllora_amd.process.canny`, cut in two at the class map (0 none, 1 weak,
2 strong); the tests first assert that the two halves composed equal `process.canny` on their inputs, so the restatement is pinned
to the shipped detector.  `ambiguous_np` marks the pixels where numpy's own sector is rounding noise: `mag >= low` and the angle,
recomputed in float64 from the fp32 gx / gy, within 1e-3 degrees of a sector boundary."""
import numpy as np

from controllora_amd.process import _conv2_same

AMBIGUOUS_DEG = 1e-3
AMBIGUOUS_CAP = 2e-4          # at most this share of an image's pixels may be ambiguous (asserted before every comparison)


def _gradients(img):
    g = img.astype(np.float32)
    if g.ndim == 3:
        g = 0.299 * g[..., 0] + 0.587 * g[..., 1] + 0.114 * g[..., 2]
    kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], np.float32)
    return _conv2_same(g, kx), _conv2_same(g, kx.T)


def classify_np(img, low, high):
    gx, gy = _gradients(img)
    mag = np.abs(gx) + np.abs(gy)
    ang = (np.rad2deg(np.arctan2(gy, gx)) + 180.0) % 180.0
    sector = ((ang + 22.5) // 45).astype(np.int32) % 4
    p = np.pad(mag, 1)
    H, W = mag.shape
    nb = {0: (p[1:H + 1, 2:], p[1:H + 1, :W]), 1: (p[2:, 2:], p[:H, :W]), 2: (p[2:, 1:W + 1], p[:H, 1:W + 1]),
          3: (p[2:, :W], p[:H, 2:])}
    keep = np.zeros_like(mag, dtype=bool)
    for s_, (a, b) in nb.items():
        keep |= (sector == s_) & (mag >= a) & (mag >= b)
    strong = keep & (mag >= high)
    weak = keep & (mag >= low)
    return weak.astype(np.uint8) + strong.astype(np.uint8)          # low <= high: strong is a subset of weak


def hysteresis_np(cls):
    strong, weak = cls == 2, cls >= 1
    out = strong.copy()
    while True:
        q = np.pad(out, 1)
        grown = weak & (q[:-2, :-2] | q[:-2, 1:-1] | q[:-2, 2:] | q[1:-1, :-2] | q[1:-1, 2:] | q[2:, :-2] | q[2:, 1:-1] | q[2:, 2:] | out)
        if (grown == out).all():
            break
        out = grown
    return out.astype(np.uint8) * 255


def hysteresis_flood(cls):
    """the same fixed point by a stack flood fill from the strong pixels (for chains too long for the loop above, which makes
    one whole-image pass per pixel of the chain); the CPU tests pin it to `hysteresis_np` on every small map"""
    H, W = cls.shape
    out = cls == 2
    weak = cls >= 1
    stack = list(zip(*np.nonzero(out)))
    while stack:
        y, x = stack.pop()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                yy, xx = y + dy, x + dx
                if 0 <= yy < H and 0 <= xx < W and weak[yy, xx] and not out[yy, xx]:
                    out[yy, xx] = True
                    stack.append((yy, xx))
    return out.astype(np.uint8) * 255


def ambiguous_np(img, low):
    gx, gy = _gradients(img)
    mag = np.abs(gx) + np.abs(gy)
    ang = np.rad2deg(np.arctan2(gy.astype(np.float64), gx.astype(np.float64))) % 180.0
    u = (ang - 22.5) % 45.0                                          # sector boundaries: 22.5 + 45 k degrees
    return (mag >= low) & (np.minimum(u, 45.0 - u) <= AMBIGUOUS_DEG)


def check_classify(got, img, low, high):
    """the staged contract, stage 1: the share of ambiguous pixels is under the cap (asserted first), and the class map equals
    numpy's at every other pixel; -> number of ambiguous pixels"""
    amb = ambiguous_np(img, low)
    assert amb.mean() <= AMBIGUOUS_CAP, (int(amb.sum()), amb.size)
    want = classify_np(img, low, high)
    bad = (got != want) & ~amb
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist())
    return int(amb.sum())


# ---------------------------------------------------------------- inputs
def _smooth(a, sigma):
    r = int(3 * sigma + 0.5)
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    for ax in (0, 1):
        a = np.apply_along_axis(lambda v: np.convolve(np.pad(v, r, mode="reflect"), k, mode="valid"), ax, a)
    return a


def noise_image(seed, H, W, C=3, sigma=0.0):
    """uint8 [H,W,C] (C = 3) or [H,W] (C = 1): uniform noise, optionally smoothed with a Gaussian and stretched back to 0 .. 255"""
    rng = np.random.default_rng(seed)
    a = rng.random((H, W, C))
    if sigma > 0:
        a = _smooth(a, sigma)
        a = (a - a.min()) / (a.max() - a.min())
    a = (a * 255.999).astype(np.uint8)
    return np.ascontiguousarray(a if C == 3 else a[..., 0])


def thresholds(seed, n):
    """n pairs drawn like the data set draws them: two integers in [1, 255), swapped where low > high"""
    rng = np.random.default_rng(1000 + seed)
    t = rng.integers(1, 255, (n, 2))
    return t.min(1).astype(np.float32), t.max(1).astype(np.float32)


def snake(H, W, strong=True, step=2):
    """class map with ONE weak chain, a serpentine of horizontal runs on every `step`-th row joined at alternating ends, and (with
    `strong`) a single strong pixel at its start: the whole chain must light up, or nothing"""
    cls = np.zeros((H, W), np.uint8)
    right = True
    for y in range(0, H, step):
        cls[y, :] = 1
        if y + step < H:
            cls[y + 1:y + step, W - 1 if right else 0] = 1
        right = not right
    if strong:
        cls[0, 0] = 2
    return cls
