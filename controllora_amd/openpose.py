"""OpenPose body detector on the HIP path: what the reference pose app runs on the user's photo
(reference apps/gradio_pose2image.py:75 `apply_openpose(resize_image(input_image, detect_resolution))`).

  BodyPoseNet       the body network of reference annotator/openpose/model.py:24-142 (`bodypose_model`) on the kernels of
                    controllora_amd/csrc/clora_pose.hip: 92 convolutions with a fused bias / ReLU and 3 max pools, fp16 NHWC
                    activations.  The two branches of a stage run as the two jobs of one launch; the concatenation
                    [L1 | L2 | features] that every stage reads (model.py:120-140) is never formed by a copy: the stage buffer is
                    [features 128 | L1 38 | L2 19 | 7 zero] = 192 channels, the branch heads store straight into it and the weights
                    of every Mconv1_stage* are packed with their input channels in that order.
  Body              reference annotator/openpose/body.py:24-209 around it, on the host in numpy: resize, pad, network, map resize,
                    peaks, part-affinity line integrals, person assembly.  `postprocess` is callable on its own.
  draw_bodypose     reference annotator/openpose/util.py:37-70 with PIL's rasteriser.
  OpenposeDetector  reference annotator/openpose/__init__.py:16-44, body only.

cv2 and torchvision are not used: the two cubic resizes are interpolation matrices applied from the left and the right."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import kernels as K

f16, f32 = torch.float16, torch.float32

# ---------------------------------------------------------------- the layer table (reference model.py:34-94), as data
# (name, Cin, Cout, ksize) or the name of a 2x2 max pool
VGG = [("conv1_1", 3, 64, 3), ("conv1_2", 64, 64, 3), "pool1_stage1", ("conv2_1", 64, 128, 3), ("conv2_2", 128, 128, 3), "pool2_stage1",
       ("conv3_1", 128, 256, 3), ("conv3_2", 256, 256, 3), ("conv3_3", 256, 256, 3), ("conv3_4", 256, 256, 3), "pool3_stage1",
       ("conv4_1", 256, 512, 3), ("conv4_2", 512, 512, 3), ("conv4_3_CPM", 512, 256, 3), ("conv4_4_CPM", 256, 128, 3)]
N_PAF, N_HEAT, N_FEAT = 38, 19, 128
STAGE_C = 192                                           # [features 128 | L1 38 | L2 19 | 7 zero]
OFF_L1, OFF_L2 = N_FEAT, N_FEAT + N_PAF                 # 128 and 166: both even, as the kernel's paired stores need


def _branch(stage: int, br: int):
    n = N_PAF if br == 1 else N_HEAT
    if stage == 1:
        return [(f"conv5_1_CPM_L{br}", 128, 128, 3), (f"conv5_2_CPM_L{br}", 128, 128, 3), (f"conv5_3_CPM_L{br}", 128, 128, 3),
                (f"conv5_4_CPM_L{br}", 128, 512, 1), (f"conv5_5_CPM_L{br}", 512, n, 1)]
    return [(f"Mconv1_stage{stage}_L{br}", 185, 128, 7)] + [(f"Mconv{i}_stage{stage}_L{br}", 128, 128, 7) for i in (2, 3, 4, 5)] + \
        [(f"Mconv6_stage{stage}_L{br}", 128, 128, 1), (f"Mconv7_stage{stage}_L{br}", 128, n, 1)]


# The layers without a ReLU.  The reference's list (model.py:29-32) names Mconv7_stage6_L1 twice and never Mconv7_stage6_L2, so the
# LAST heat-map layer DOES get a ReLU there: the final heat maps are clipped at 0.  That quirk is kept (and pinned by a test).
NO_RELU = {"conv5_5_CPM_L1", "conv5_5_CPM_L2"} | {f"Mconv7_stage{s}_L{b}" for s in range(2, 7) for b in (1, 2)} - {"Mconv7_stage6_L2"}


def layer_table():
    """every layer in execution order: dicts name, module (the reference's Sequential: model0, model<stage>_<branch>), and for a
    convolution Cin, Cout, ksize, relu; pools have ksize 0"""
    rows = []
    for item in VGG:
        if isinstance(item, str):
            rows.append(dict(name=item, module="model0", ksize=0))
        else:
            n, ci, co, k = item
            rows.append(dict(name=n, module="model0", Cin=ci, Cout=co, ksize=k, relu=n not in NO_RELU))
    for s in range(1, 7):
        for br in (1, 2):
            for n, ci, co, k in _branch(s, br):
                rows.append(dict(name=n, module=f"model{s}_{br}", Cin=ci, Cout=co, ksize=k, relu=n not in NO_RELU))
    return rows


def concat_permutation() -> list:
    """source channel of the reference's concatenation [L1 38 | L2 19 | features 128] (model.py:120) for every channel of the stage
    buffer [features 128 | L1 38 | L2 19 | 7 pad]; -1 = pad"""
    return [N_PAF + N_HEAT + c for c in range(N_FEAT)] + list(range(N_PAF + N_HEAT)) + [-1] * (STAGE_C - 185)


def random_state_dict(seed: int = 0) -> dict:
    """`random:openpose`: He-initialised weights (std sqrt(2 / fan_in), zero bias) so activations stay O(1) through 50 layers"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for L in layer_table():
        if L["ksize"]:
            fan = L["Cin"] * L["ksize"] ** 2
            sd[L["name"] + ".weight"] = torch.randn(L["Cout"], L["Cin"], L["ksize"], L["ksize"], generator=g) * math.sqrt(2.0 / fan)
            sd[L["name"] + ".bias"] = torch.zeros(L["Cout"])
    return sd


class BodyPoseNet:
    def __init__(self, state_dict: Optional[dict] = None, device="cuda"):
        self.device = torch.device(device)
        self.layers = layer_table()
        self.convs = {L["name"]: L for L in self.layers if L["ksize"]}
        self.weights, self.packed, self.bias = {}, {}, {}
        self._bufs = {}
        self.launches = 0
        self.splits = {}                  # layer name -> K ranges of its launch, recorded by forward(return_activations=True)
        if state_dict is not None:
            self.load_state_dict(state_dict)

    @classmethod
    def from_pretrained(cls, path: str, device="cuda", seed: int = 0):
        """a `.pth` file (the converted Caffe weights, body_pose_model.pth) or `random:openpose`, the offline stand-in"""
        if path == "random:openpose":
            return cls(random_state_dict(seed), device)
        return cls(torch.load(path, map_location="cpu", weights_only=True), device)

    def load_state_dict(self, sd: dict):
        """bare layer names (`conv1_1.weight`, the converted Caffe file) or module-prefixed ones (`model0.conv1_1.weight`, what the
        reference's util.transfer maps to, util.py:30-34)"""
        got = {}
        for key, t in sd.items():
            parts = key.split(".")
            if len(parts) < 2 or parts[-1] not in ("weight", "bias"):
                raise KeyError(f"unexpected key {key!r}")
            if len(parts) == 3 and self.convs.get(parts[1], {}).get("module") != parts[0]:
                raise KeyError(f"{key!r}: layer {parts[1]} does not live in {parts[0]}")
            got[".".join(parts[-2:])] = t
        want = {f"{n}.{k}" for n in self.convs for k in ("weight", "bias")}
        if set(got) != want:
            raise KeyError(f"missing {sorted(want - set(got))[:4]}, unexpected {sorted(set(got) - want)[:4]}")
        perm = torch.tensor(concat_permutation(), dtype=torch.int32, device=self.device)
        for n, L in self.convs.items():
            w, b = got[n + ".weight"].detach().float().contiguous(), got[n + ".bias"].detach().float().contiguous()
            if tuple(w.shape) != (L["Cout"], L["Cin"], L["ksize"], L["ksize"]) or tuple(b.shape) != (L["Cout"],):
                raise ValueError(f"{n}: weight {tuple(w.shape)} bias {tuple(b.shape)}")
            self.weights[n + ".weight"], self.weights[n + ".bias"] = w.cpu(), b.cpu()
            L["CinK"] = STAGE_C if L["Cin"] == 185 else (L["Cin"] + 7) // 8 * 8          # kernel-side input channels
            self.packed[n] = K.conv_act_pack(w.to(self.device), L["CinK"], perm if L["Cin"] == 185 else None)   # one launch per layer
            self.bias[n] = b.to(self.device)
        return self

    def state_dict(self) -> dict:
        return dict(self.weights)

    # ---- buffers: two ping-pong activations and the stage buffer, per input size
    def _buffers(self, B, H, W):
        key = (B, H, W)
        if key not in self._bufs:
            n = B * H * W * 64                                              # the widest activation: 64 channels at full size
            self._bufs = {key: (torch.empty(n, dtype=f16, device=self.device), torch.empty(n, dtype=f16, device=self.device),
                                torch.zeros(B * (H // 8) * (W // 8), STAGE_C, dtype=f16, device=self.device))}   # zeroed once: finite pads
        return self._bufs[key]

    def _conv(self, names, xs, ys, B, H, W):
        jobs = []
        for n, x, y in zip(names, xs, ys):
            L = self.convs[n]
            jobs.append(dict(x=x, w=self.packed[n], bias=self.bias[n], y=y, Cin=L["CinK"], Cout=L["Cout"], relu=L["relu"]))
        k = self.convs[names[0]]["ksize"]
        if self._record:
            self.splits.update({n: K.conv_act_splits(jobs, B, H, W, k) for n in names})
        self.launches += K.conv_act(jobs, B, H, W, k)

    def forward(self, x: torch.Tensor, return_activations: bool = False):
        """x fp16 [B, 3, H, W] on the device, H and W multiples of 8 -> (paf [B, 38, H/8, W/8], heat [B, 19, H/8, W/8]) fp16;
        with `return_activations` also {layer name: its output, fp16 NHWC [B, h, w, C]} for all 92 convolutions and 3 pools"""
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype != f16 or x.shape[2] % 8 or x.shape[3] % 8 or x.device.type != self.device.type:
            raise ValueError(f"expected fp16 [B, 3, H, W] on {self.device} with H, W % 8 == 0, got {x.dtype} {tuple(x.shape)} on {x.device}")
        B, _, H, W = x.shape
        a, b, stage = self._buffers(B, H, W)
        self.launches, self._record = 0, return_activations
        acts = {}
        cur = torch.zeros(B * H * W, 8, dtype=f16, device=self.device)       # the image, NHWC, 3 -> 8 channels
        cur[:, :3] = x.permute(0, 2, 3, 1).reshape(-1, 3)
        h, w = H, W

        def view(buf, rows, C, ld=None, off=0):
            ld = C if ld is None else ld
            return buf[:rows * ld].view(rows, ld)[:, off:off + C]

        def keep(name, t, hh, ww):
            if return_activations:
                acts[name] = t.reshape(B, hh, ww, t.shape[-1]).clone()

        for L in self.layers[:len(VGG)]:
            dst = b if cur.data_ptr() == a.data_ptr() else a
            if L["ksize"] == 0:
                C = cur.shape[1]
                out = view(dst, B * (h // 2) * (w // 2), C)
                K.maxpool2x2(cur.reshape(B, h, w, C), out=out.view(B, h // 2, w // 2, C))
                self.launches += 1
                h, w = h // 2, w // 2
            else:
                rows = B * h * w
                out = stage[:, :N_FEAT] if L["name"] == "conv4_4_CPM" else view(dst, rows, L["Cout"])     # features: straight into the stage buffer
                self._conv([L["name"]], [cur], [out], B, h, w)
            keep(L["name"], out, h, w)
            cur = out
        rows = B * h * w
        for s in range(1, 7):
            names = [[n for n, *_ in _branch(s, br)] for br in (1, 2)]
            xs = [stage[:, :N_FEAT]] * 2 if s == 1 else [stage] * 2
            src = None
            for i, pair in enumerate(zip(*names)):
                C = self.convs[pair[0]]["Cout"]
                if i == len(names[0]) - 1:                                   # the heads: beside the features, for the next stage to read
                    ys = [stage[:, OFF_L1:OFF_L1 + N_PAF], stage[:, OFF_L2:OFF_L2 + N_HEAT]]
                else:
                    dst = b if src is a else a
                    ys = [view(dst, rows, C, 2 * C, 0), view(dst, rows, C, 2 * C, C)]
                    src = dst
                self._conv(pair, xs, ys, B, h, w)
                for n, y in zip(pair, ys):
                    keep(n, y, h, w)
                xs = ys
        paf = stage[:, OFF_L1:OFF_L1 + N_PAF].reshape(B, h, w, N_PAF).permute(0, 3, 1, 2).contiguous()
        heat = stage[:, OFF_L2:OFF_L2 + N_HEAT].reshape(B, h, w, N_HEAT).permute(0, 3, 1, 2).contiguous()
        return (paf, heat, acts) if return_activations else (paf, heat)

    __call__ = forward


# ---------------------------------------------------------------- resizes (cv2.resize INTER_CUBIC as matrices)
def cubic_taps(t):
    """the four Keys weights (a = -0.75, OpenCV's bicubic) of the samples at -1, 0, 1, 2 for a phase t in [0, 1)"""
    a = -0.75
    w0 = ((a * (t + 1) - 5 * a) * (t + 1) + 8 * a) * (t + 1) - 4 * a
    w1 = ((a + 2) * t - (a + 3)) * t * t + 1
    w2 = ((a + 2) * (1 - t) - (a + 3)) * (1 - t) * (1 - t) + 1
    return np.stack([w0, w1, w2, 1.0 - w0 - w1 - w2], -1)


def cubic_matrix(n_src: int, n_dst: int, inv_scale: Optional[float] = None) -> np.ndarray:
    """[n_dst, n_src]: destination pixel d samples the source at (d + 0.5) * inv_scale - 0.5 (pixel-centre alignment) with the four
    Keys taps; indices past the border take the border pixel (replicate).  inv_scale defaults to n_src / n_dst (a given size); a
    resize by a factor f passes 1 / f, as cv2.resize does."""
    inv = n_src / n_dst if inv_scale is None else inv_scale
    s = (np.arange(n_dst) + 0.5) * inv - 0.5
    i0 = np.floor(s).astype(np.int64)
    taps = cubic_taps(s - i0)
    R = np.zeros((n_dst, n_src))
    for k in range(4):
        np.add.at(R, (np.arange(n_dst), np.clip(i0 - 1 + k, 0, n_src - 1)), taps[:, k])
    return R


def resize_cubic(img: np.ndarray, Ry: np.ndarray, Rx: np.ndarray) -> np.ndarray:
    """Ry @ img @ Rx^T per channel, float64"""
    a = np.asarray(img, np.float64)
    if a.ndim == 2:
        return Ry @ a @ Rx.T
    return np.einsum("ij,jkc,lk->ilc", Ry, a, Rx, optimize=True)


def to_uint8(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def map_resize_matrices(h, w, pad_down, pad_right, H, W, stride=8):
    """the chain body.py:55-57 applies to a network map [h, w]: x8 cubic, crop the pad, cubic to the photo's [H, W] -> (My [H, h], Mx [W, w])"""
    def one(n, pad, N):
        up = cubic_matrix(n, n * stride, 1.0 / stride)[:n * stride - pad]
        return cubic_matrix(n * stride - pad, N) @ up
    return one(h, pad_down, H), one(w, pad_right, W)


# ---------------------------------------------------------------- post-processing (body.py:68-209)
LIMB_SEQ = [[2, 3], [2, 6], [3, 4], [4, 5], [6, 7], [7, 8], [2, 9], [9, 10], [10, 11], [2, 12], [12, 13], [13, 14], [2, 1], [1, 15],
            [15, 17], [1, 16], [16, 18], [3, 17], [6, 18]]
MAP_IDX = [[31, 32], [39, 40], [33, 34], [35, 36], [41, 42], [43, 44], [19, 20], [21, 22], [23, 24], [25, 26], [27, 28], [29, 30],
           [47, 48], [49, 50], [53, 54], [51, 52], [55, 56], [37, 38], [45, 46]]
COLORS = [[255, 0, 0], [255, 85, 0], [255, 170, 0], [255, 255, 0], [170, 255, 0], [85, 255, 0], [0, 255, 0], [0, 255, 85], [0, 255, 170],
          [0, 255, 255], [0, 170, 255], [0, 85, 255], [0, 0, 255], [85, 0, 255], [170, 0, 255], [255, 0, 255], [255, 0, 170], [255, 0, 85]]
THRE1, THRE2, MID_NUM = 0.1, 0.05, 10


def find_peaks(heat_full):
    """body.py:71-92: per part, the pixels of the sigma-3 smoothed map that are >= their 4 neighbours (zero outside) and > 0.1;
    -> per part a list of (x, y, score of the unsmoothed map, id)"""
    from scipy.ndimage import gaussian_filter
    all_peaks, counter = [], 0
    for part in range(18):
        ori = heat_full[:, :, part]
        sm = gaussian_filter(ori, sigma=3)
        p = np.pad(sm, 1)
        binary = (sm >= p[:-2, 1:-1]) & (sm >= p[2:, 1:-1]) & (sm >= p[1:-1, :-2]) & (sm >= p[1:-1, 2:]) & (sm > THRE1)
        ys, xs = np.nonzero(binary)
        all_peaks.append([(int(x), int(y), float(ori[y, x]), counter + i) for i, (x, y) in enumerate(zip(xs, ys))])
        counter += len(xs)
    return all_peaks


def connect_limbs(all_peaks, paf_full):
    """body.py:103-152: for every limb the part-affinity line integral over 10 samples between every pair of candidate joints, the
    0.05 / 80 % / distance-prior criteria, then a greedy one-to-one assignment by descending score"""
    H = paf_full.shape[0]
    connection_all, special = [], []
    for k in range(len(MAP_IDX)):
        score_mid = paf_full[:, :, [x - 19 for x in MAP_IDX[k]]]
        candA, candB = all_peaks[LIMB_SEQ[k][0] - 1], all_peaks[LIMB_SEQ[k][1] - 1]
        nA, nB = len(candA), len(candB)
        if nA == 0 or nB == 0:
            special.append(k)
            connection_all.append([])
            continue
        A, Bq = np.array([c[:2] for c in candA], np.float64), np.array([c[:2] for c in candB], np.float64)
        vec = Bq[None, :, :] - A[:, None, :]                                           # [nA, nB, 2]
        norm = np.maximum(0.001, np.sqrt((vec ** 2).sum(-1)))
        vec = vec / norm[..., None]
        step = (Bq[None, :, :] - A[:, None, :]) / (MID_NUM - 1)                       # np.linspace: arange * step + start, the end exact
        pts = np.arange(MID_NUM)[None, None, :, None] * step[:, :, None, :] + A[:, None, None, :]
        pts[:, :, -1] = Bq[None, :, :]
        xi, yi = np.rint(pts[..., 0]).astype(np.int64), np.rint(pts[..., 1]).astype(np.int64)
        mid = score_mid[yi, xi]                                                        # [nA, nB, 10, 2]
        score_midpts = mid[..., 0] * vec[..., None, 0] + mid[..., 1] * vec[..., None, 1]
        prior = score_midpts.sum(-1) / MID_NUM + np.minimum(0.5 * H / norm - 1, 0)
        ok = ((score_midpts > THRE2).sum(-1) > 0.8 * MID_NUM) & (prior > 0)
        cand = [(int(i), int(j), float(prior[i, j])) for i, j in zip(*np.nonzero(ok))]
        cand = sorted(cand, key=lambda c: c[2], reverse=True)
        connection, usedA, usedB = [], set(), set()
        for i, j, s in cand:
            if i not in usedA and j not in usedB:
                connection.append([candA[i][3], candB[j][3], s, i, j])
                usedA.add(i)
                usedB.add(j)
                if len(connection) >= min(nA, nB):
                    break
        connection_all.append(np.array(connection, np.float64).reshape(-1, 5))
    return connection_all, special


def assemble(all_peaks, connection_all, special):
    """body.py:154-209: limbs that share a joint join one person; two people that a limb links merge when they share no part; people
    with fewer than 4 parts or a mean score below 0.4 are deleted"""
    subset = -1 * np.ones((0, 20))
    candidate = np.array([item for sub in all_peaks for item in sub], np.float64).reshape(-1, 4)
    for k in range(len(MAP_IDX)):
        if k in special:
            continue
        conn = connection_all[k]
        indexA, indexB = np.array(LIMB_SEQ[k]) - 1
        for i in range(len(conn)):
            pa, pb, sc = conn[i][0], conn[i][1], conn[i][2]
            found = [j for j in range(len(subset)) if subset[j][indexA] == pa or subset[j][indexB] == pb][:2]
            if len(found) == 1:
                j = found[0]
                if subset[j][indexB] != pb:
                    subset[j][indexB] = pb
                    subset[j][-1] += 1
                    subset[j][-2] += candidate[int(pb), 2] + sc
            elif len(found) == 2:
                j1, j2 = found
                membership = ((subset[j1] >= 0).astype(int) + (subset[j2] >= 0).astype(int))[:-2]
                if not (membership == 2).any():
                    subset[j1][:-2] += subset[j2][:-2] + 1
                    subset[j1][-2:] += subset[j2][-2:]
                    subset[j1][-2] += sc
                    subset = np.delete(subset, j2, 0)
                else:
                    subset[j1][indexB] = pb
                    subset[j1][-1] += 1
                    subset[j1][-2] += candidate[int(pb), 2] + sc
            elif k < 17:
                row = -1 * np.ones(20)
                row[indexA], row[indexB] = pa, pb
                row[-1] = 2
                row[-2] = candidate[int(pa), 2] + candidate[int(pb), 2] + sc
                subset = np.vstack([subset, row])
    drop = [i for i in range(len(subset)) if subset[i][-1] < 4 or subset[i][-2] / subset[i][-1] < 0.4]
    return candidate, np.delete(subset, drop, axis=0)


def postprocess(heat_full: np.ndarray, paf_full: np.ndarray):
    """heat maps [H, W, 19] and part-affinity fields [H, W, 38] at the photo's resolution -> (candidate [n, 4]: x, y, score, id;
    subset [p, 20]: per person the candidate index of each of the 18 parts or -1, the total score, the number of parts)"""
    heat_full, paf_full = np.asarray(heat_full, np.float64), np.asarray(paf_full, np.float64)
    peaks = find_peaks(heat_full)
    conn, special = connect_limbs(peaks, paf_full)
    return assemble(peaks, conn, special)


class Body:
    """reference annotator/openpose/body.py:14-209 with one scale (the reference's scale_search is [0.5], body.py:26)"""
    STRIDE, PAD_VALUE = 8, 128

    def __init__(self, net: BodyPoseNet, boxsize: int = 368):
        self.net = net
        self.BOXSIZE = boxsize            # body.py:27; the photo is resized to half of it in height (smaller only in tests on the emulator)
        self.timings = {}

    def maps(self, bgr: np.ndarray):
        """photo uint8 [H, W, 3] -> (heat [H, W, 19], paf [H, W, 38]) float64 at the photo's resolution (body.py:32-66; with one scale
        `heatmap_avg += heatmap_avg + heatmap / 1` on a zero array is the map itself)"""
        H, W = bgr.shape[:2]
        scale = 0.5 * self.BOXSIZE / H
        h1, w1 = int(np.rint(H * scale)), int(np.rint(W * scale))
        small = to_uint8(resize_cubic(bgr, cubic_matrix(H, h1, 1.0 / scale), cubic_matrix(W, w1, 1.0 / scale)))
        pd, pr = (-h1) % self.STRIDE, (-w1) % self.STRIDE                    # util.py:7-27 padRightDownCorner
        padded = np.full((h1 + pd, w1 + pr, 3), self.PAD_VALUE, np.uint8)
        padded[:h1, :w1] = small
        x = torch.from_numpy(np.ascontiguousarray(padded.transpose(2, 0, 1)[None].astype(np.float32) / 256 - 0.5))
        paf, heat = self.net(x.to(self.net.device).half())
        paf, heat = paf[0].permute(1, 2, 0).float().cpu().numpy(), heat[0].permute(1, 2, 0).float().cpu().numpy()
        My, Mx = map_resize_matrices(heat.shape[0], heat.shape[1], pd, pr, H, W, self.STRIDE)
        return resize_cubic(heat, My, Mx), resize_cubic(paf, My, Mx)

    def __call__(self, bgr: np.ndarray):
        import time
        t0 = time.perf_counter()
        heat, paf = self.maps(bgr)
        t1 = time.perf_counter()
        out = postprocess(heat, paf)
        self.timings = {"maps_s": t1 - t0, "postprocess_s": time.perf_counter() - t1}
        return out


# ---------------------------------------------------------------- drawing (util.py:37-70)
def add_weighted(a, wa, b, wb):
    """cv2.addWeighted on uint8: round to nearest even, saturate"""
    return np.clip(np.rint(a.astype(np.float64) * wa + b.astype(np.float64) * wb), 0, 255).astype(np.uint8)


def ellipse_polygon(cx, cy, ax, ay, angle):
    """cv2.ellipse2Poly(center, axes, angle, 0, 360, 1): the rounded points of the rotated ellipse in 1-degree steps"""
    t = np.deg2rad(np.arange(0, 361))
    ca, sa = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    x = cx + ax * np.cos(t) * ca - ay * np.sin(t) * sa
    y = cy + ax * np.cos(t) * sa + ay * np.sin(t) * ca
    return [(int(px), int(py)) for px, py in zip(np.rint(x), np.rint(y))]


def draw_bodypose(canvas: np.ndarray, candidate, subset) -> np.ndarray:
    """Filled radius-4 discs at the joints in the 18 colours, then every limb as a filled ellipse polygon (half-axes int(length / 2)
    and 4, integer angle, 1-degree steps), each blended onto the canvas with 0.4 * canvas + 0.6 * drawn.  Rasterised with PIL's
    ImageDraw: equality with OpenCV's rasteriser on the boundary pixels of discs and polygons is NOT claimed and not checked (OpenCV
    is not a dependency of this project and no test can call it); interiors, colours, blend arithmetic and order are the reference's."""
    from PIL import Image, ImageDraw
    candidate, subset = np.asarray(candidate, np.float64).reshape(-1, 4), np.asarray(subset, np.float64).reshape(-1, 20)
    img = Image.fromarray(np.ascontiguousarray(canvas))
    d = ImageDraw.Draw(img)
    for i in range(18):
        for person in subset:
            idx = int(person[i])
            if idx == -1:
                continue
            x, y = int(candidate[idx][0]), int(candidate[idx][1])
            d.ellipse([x - 4, y - 4, x + 4, y + 4], fill=tuple(COLORS[i]))
    canvas = np.array(img)
    for i in range(17):
        for person in subset:
            index = person[np.array(LIMB_SEQ[i]) - 1]
            if -1 in index:
                continue
            xs, ys = candidate[index.astype(int), 0], candidate[index.astype(int), 1]
            length = ((xs[0] - xs[1]) ** 2 + (ys[0] - ys[1]) ** 2) ** 0.5
            angle = math.degrees(math.atan2(ys[0] - ys[1], xs[0] - xs[1]))
            cur = Image.fromarray(canvas)
            ImageDraw.Draw(cur).polygon(ellipse_polygon(int(np.mean(xs)), int(np.mean(ys)), int(length / 2), 4, int(angle)), fill=tuple(COLORS[i]))
            canvas = add_weighted(canvas, 0.4, np.array(cur), 0.6)
    return canvas


class OpenposeDetector:
    """reference annotator/openpose/__init__.py:16-44, body only: `detector(rgb_uint8) -> (canvas, {"candidate": ..., "subset": ...})`"""

    def __init__(self, weights: str = "random:openpose", device="cuda", boxsize: int = 368):
        self.body_estimation = Body(BodyPoseNet.from_pretrained(weights, device), boxsize)

    def __call__(self, rgb: np.ndarray, hand: bool = False):
        if hand:
            raise NotImplementedError("the hand model is not part of this detector (neither reference app passes hand=True)")
        bgr = np.ascontiguousarray(rgb[:, :, ::-1])
        candidate, subset = self.body_estimation(bgr)
        canvas = draw_bodypose(np.zeros_like(bgr), candidate, subset)
        return canvas, dict(candidate=candidate.tolist(), subset=subset.tolist())
