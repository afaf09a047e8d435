"""Shared cases of the OpenPose tests (tests/test_openpose_emu.py, tests/test_openpose_gpu.py, tests/test_openpose_cpu.py,
tests/test_openpose_mutants_emu.py): the kernel cases of controllora_amd/csrc/clora_pose.hip, a plain-torch restatement of the body
network (reference annotator/openpose/model.py `bodypose_model`), the network checks and the planted-skeleton generator.

Kernel cases: outputs start as NaN, the reference is the fp64 convolution of the same fp16-rounded operands, every element has the
derived limit of tests/kernel_cases.py `within_limit` with L = ksize^2 Cin + splits + 1 accumulation steps (the K terms, the fp32 sum of
the split-K slabs, the bias), `mag` = the convolution of the absolute values plus |bias|, the fp16 rounding term taken from the
pre-activation value (|relu a - relu b| <= |a - b|); `no_outliers` beside it; a second launch must give the same bits."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from controllora_amd import capi, kernels as K, openpose as OP
from tests import kernel_cases as KC

f16, f32, f64 = torch.float16, torch.float32, torch.float64


# ---------------------------------------------------------------- kernel cases
@functools.lru_cache(maxsize=8)
def _conv_problem(B, H, W, Cin, Cout, k, seed):
    """x fp16 [B,H,W,Cin], w fp32 OIHW, bias fp32, and on the CPU in fp64: the pre-activation reference and the magnitude"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, Cin, generator=g).half()
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    bias = torch.randn(Cout, generator=g) * 0.5
    x64, w64 = x.double().permute(0, 3, 1, 2), w.half().double()
    pre = F.conv2d(x64, w64, bias.double(), padding=k // 2)
    mag = F.conv2d(x64.abs(), w64.abs(), bias.double().abs(), padding=k // 2)
    return x, w, bias, KC.nhwc(pre).contiguous(), KC.nhwc(mag).contiguous()


def case_conv_act(dev, B, H, W, Cin, Cout, k, relus=(True,), seed=0):
    """len(relus) jobs in one launch, job j with its own input, weights (seed + j), bias and ReLU flag"""
    rows = B * H * W
    probs = [_conv_problem(B, H, W, Cin, Cout, k, seed + j) for j in range(len(relus))]
    jobs, outs = [], []
    for (x, w, bias, _, _), relu in zip(probs, relus):
        outs.append(KC.nan_out(rows, Cout, dev))
        jobs.append(dict(x=x.to(dev).reshape(rows, Cin), w=K.conv_act_pack(w.to(dev), Cin), bias=bias.to(dev), y=outs[-1], Cin=Cin, Cout=Cout,
                         relu=relu))
    splits = K.conv_act_splits(jobs, B, H, W, k)
    K.conv_act(jobs, B, H, W, k)
    first = [o.clone() for o in outs]
    what = f"conv_act {k}x{k} {(B, H, W, Cin, Cout)} jobs {len(relus)} splits {splits}"
    for j, ((_, _, _, pre, mag), relu) in enumerate(zip(probs, relus)):
        ref = pre.clamp_min(0) if relu else pre
        KC.within_limit(first[j], ref, mag, k * k * Cin + splits + 1, rounded=[pre], what=f"{what}: job {j} relu {relu}")
        KC.no_outliers(first[j], ref, what)
        if relu:
            assert float(first[j].float().min()) >= 0 and float(pre.min()) < 0, what
        else:
            assert float(first[j].float().min()) < 0, what
    for o in outs:
        o.fill_(float("nan"))
    K.conv_act(jobs, B, H, W, k)
    for a, b in zip(first, outs):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{what}: a second launch gave other bits"
    return splits


SENTINEL = 0x5A5A          # bit pattern of the stage buffer before the heads store into it


def case_heads(dev, B, H, W, seed=40):
    """the 1x1 heads of a stage as ONE two-job launch into a 192-pitch buffer: Cout 38 at channel 128, Cout 19 at channel 166, every
    other channel keeps the sentinel bit for bit"""
    rows, Cin = B * H * W, 128
    buf = torch.full((rows, OP.STAGE_C), SENTINEL, dtype=torch.int16).view(f16).to(dev)
    jobs, probs = [], []
    for j, (off, Cout, relu) in enumerate(((OP.OFF_L1, OP.N_PAF, False), (OP.OFF_L2, OP.N_HEAT, True))):
        x, w, bias, pre, mag = _conv_problem(B, H, W, Cin, Cout, 1, seed + j)
        probs.append((off, Cout, relu, pre, mag))
        jobs.append(dict(x=x.to(dev).reshape(rows, Cin), w=K.conv_act_pack(w.to(dev), Cin), bias=bias.to(dev), y=buf[:, off:off + Cout], Cin=Cin,
                         Cout=Cout, relu=relu))
    splits = K.conv_act_splits(jobs, B, H, W, 1)
    K.conv_act(jobs, B, H, W, 1)
    got = buf.cpu()
    bits = got.view(torch.int16)
    keep = torch.ones(OP.STAGE_C, dtype=torch.bool)
    for off, Cout, relu, pre, mag in probs:
        keep[off:off + Cout] = False
        ref = pre.clamp_min(0) if relu else pre
        KC.within_limit(got[:, off:off + Cout], ref, mag, Cin + splits + 1, rounded=[pre], what=f"heads {(B, H, W)} splits {splits}: Cout {Cout} at {off}")
    touched = (bits[:, keep] != SENTINEL)
    assert not touched.any(), f"heads {(B, H, W)}: {int(touched.sum())} elements outside the two channel ranges were written"
    return splits


def raw_conv_act(L, jobs, B, H, W, k, njobs=None, ws=None):
    """the return code of the entry point itself (the wrapper would raise)"""
    arr = (capi.ConvActJob * max(1, len(jobs)))()
    for i, j in enumerate(jobs):
        arr[i] = capi.ConvActJob(j["x"].data_ptr(), j["x"].stride(0), j["w"].data_ptr(), j["bias"].data_ptr(), j["y"].data_ptr(), j["y"].stride(0),
                                 j["Cin"], j["Cout"], 1)
    return L.cdll.clora_conv_act_f16(arr, len(jobs) if njobs is None else njobs, B, H, W, k, ws.data_ptr() if ws is not None else None,
                                     ws.numel() if ws is not None else 0, capi.stream())


def case_rejects(dev):
    """odd channel offset, ksize outside {1, 3, 7}, Cin % 8 != 0, njobs outside 1 .. 2, a missing workspace: refused before any launch
    (the output keeps its NaNs)"""
    L = capi.lib()
    B, H, W, Cin, Cout = 1, 4, 4, 32, 20
    rows = B * H * W
    x = torch.zeros(rows, 64, dtype=f16, device=dev)
    buf = KC.nan_out(rows, 64, dev)
    bias = torch.zeros(Cout, dtype=f32, device=dev)
    w = torch.zeros(K.conv_act_packed_numel(Cout, 64, 7), dtype=f16, device=dev)
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=dev)

    def job(**kw):
        j = dict(x=x[:, :Cin], w=w, bias=bias, y=buf[:, 2:2 + Cout], Cin=Cin, Cout=Cout)
        j.update(kw)
        return j
    assert raw_conv_act(L, [job()], B, H, W, 3, ws=ws) == capi.OK
    buf.fill_(float("nan"))
    assert raw_conv_act(L, [job(y=buf[:, 3:3 + Cout])], B, H, W, 3, ws=ws) == capi.ERR_ARG          # odd channel offset
    assert raw_conv_act(L, [job()], B, H, W, 5, ws=ws) == capi.ERR_ARG
    assert raw_conv_act(L, [job()], B, H, W, 2, ws=ws) == capi.ERR_ARG
    assert raw_conv_act(L, [job(Cin=28)], B, H, W, 3, ws=ws) == capi.ERR_ARG
    assert raw_conv_act(L, [job(x=x[:, 4:4 + Cin])], B, H, W, 3, ws=ws) == capi.ERR_ARG             # input not 16-byte aligned
    assert raw_conv_act(L, [job()], B, H, W, 3, njobs=0, ws=ws) == capi.ERR_ARG
    assert raw_conv_act(L, [job(), job(), job()], B, H, W, 3, ws=ws) == capi.ERR_ARG
    assert raw_conv_act(L, [job()], B, H, W, 3, ws=None) == capi.ERR_WORKSPACE                        # 1 tile x 1 x 1 job: split, needs slabs
    if dev != "cpu":
        torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()), "a refused call wrote something"
    p = torch.zeros(1, 5, 4, 8, dtype=f16, device=dev)
    assert L.cdll.clora_maxpool2x2_f16(p.data_ptr(), p.data_ptr(), 1, 5, 4, 8, capi.stream()) == capi.ERR_ARG      # odd H
    assert L.cdll.clora_maxpool2x2_f16(p.data_ptr(), p.data_ptr(), 1, 4, 5, 8, capi.stream()) == capi.ERR_ARG      # odd W
    assert L.cdll.clora_maxpool2x2_f16(p.data_ptr(), p.data_ptr(), 1, 4, 4, 4, capi.stream()) == capi.ERR_ARG      # C % 8


def case_maxpool(dev, B, H, W, C, seed=50):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, C, generator=g).half()
    x[0, :2, :2, 0] = torch.tensor([[-0.0, 0.0], [0.0, -0.0]], dtype=f16)
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous()
    got = K.maxpool2x2(x.to(dev)).cpu()
    assert got.shape == want.shape and torch.equal(got.view(torch.int16), want.view(torch.int16)), f"maxpool {(B, H, W, C)}"


def case_pack(dev, Cout=20, CinSrc=13, CinDst=40, k=3, seed=60):
    """a permuted, padded pack, unpacked on the host, equals the fp16 rounding of the permuted weights"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(Cout, CinSrc, k, k, generator=g)
    perm = torch.full((CinDst,), -1, dtype=torch.int32)
    perm[torch.randperm(CinDst, generator=g)[:CinSrc]] = torch.randperm(CinSrc, generator=g).int()
    for pm in (perm, None):
        out = K.conv_act_pack(w.to(dev), CinDst, pm.to(dev) if pm is not None else None).cpu()
        Cin32, CoutP = (CinDst + 31) // 32 * 32, (Cout + 15) // 16 * 16
        un = out.view(k * k, Cin32 // 8, CoutP, 8).permute(2, 1, 3, 0).reshape(CoutP, Cin32, k, k)     # [co][c][tap]
        want = torch.zeros(CoutP, Cin32, k, k, dtype=f16)
        for c in range(CinDst):
            s = int(pm[c]) if pm is not None else (c if c < CinSrc else -1)
            if s >= 0:
                want[:Cout, c] = w[:, s].half()
        assert torch.equal(un.view(torch.int16), want.view(torch.int16)), "pack"
        assert (un[:Cout, :CinDst] != 0).any()


# emulator shapes (the first of each line of the issue) and GPU shapes
CONV7 = [(1, 5, 7, 192, 128), (2, 13, 9, 128, 128), (1, 23, 23, 128, 128), (16, 23, 23, 192, 128)]
CONV3 = [(1, 8, 8, 8, 64), (2, 12, 20, 64, 128), (1, 46, 46, 256, 512)]
CONV1 = [(1, 5, 7, 128, 512), (1, 23, 23, 512, 38)]
POOLS = [(2, 8, 12, 64), (1, 184, 184, 64)]


# ---------------------------------------------------------------- the network, restated in plain torch
class RefBodyPose:
    """reference model.py:24-142 restated with F.conv2d / F.max_pool2d.  `state_dict()` has the reference's module-prefixed keys.
    regime "fp32": plain fp32.  regime "fp16s": every layer's operands (input, weights) and output rounded to fp16, accumulation and
    bias in fp64 -- the arithmetic the kernels implement, without their accumulation error."""

    def __init__(self, bare_state_dict):
        self.table = OP.layer_table()
        self.params = {}
        for L in self.table:
            if L["ksize"]:
                for kind in ("weight", "bias"):
                    self.params[f"{L['module']}.{L['name']}.{kind}"] = bare_state_dict[f"{L['name']}.{kind}"].detach().float()

    def state_dict(self):
        return dict(self.params)

    def layer(self, L, x, regime):
        if L["ksize"] == 0:
            return F.max_pool2d(x, kernel_size=2, stride=2, padding=0)
        w, b = self.params[f"{L['module']}.{L['name']}.weight"], self.params[f"{L['module']}.{L['name']}.bias"]
        if regime == "fp16s":
            x, w, b = x.half().double(), w.half().double(), b.double()
        elif regime == "fp64":
            x, w, b = x.double(), w.half().double(), b.double()
        y = F.conv2d(x, w, b, stride=1, padding=L["ksize"] // 2)
        if L["relu"]:
            y = F.relu(y)
        return y.half().double() if regime == "fp16s" else y

    def forward(self, x, regime="fp32"):
        x = x.float() if regime == "fp32" else x.double()
        by_module = {}
        for L in self.table:
            by_module.setdefault(L["module"], []).append(L)
        for L in by_module["model0"]:
            x = self.layer(L, x, regime)
        feat, inp = x, x
        for s in range(1, 7):
            outs = []
            for br in (1, 2):
                y = inp
                for L in by_module[f"model{s}_{br}"]:
                    y = self.layer(L, y, regime)
                outs.append(y)
            inp = torch.cat([outs[0], outs[1], feat], 1)                  # model.py:120 ... 140
        return outs[0], outs[1]


def net_input(B, H, W, seed=7):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 3, H, W, generator=g) - 0.5).half()          # the range of the detector's `x / 256 - 0.5`


def check_layerwise(net, x, acts):
    """every layer's output against the fp64 operation applied to the PRODUCT's own input of that layer (its previous activation, or
    the concatenation in the reference's channel order with the unpermuted weights): within_limit, nothing measured; -> layers checked"""
    ref = RefBodyPose(net.state_dict())
    nchw = lambda t: t.cpu().double().permute(0, 3, 1, 2)
    n_conv = n_pool = 0
    prev, feat, heads = x.cpu().double(), None, {}
    for L in ref.table:
        name = L["name"]
        stage = 0 if L["module"] == "model0" else int(L["module"][5])
        if name.startswith("conv5_1_CPM"):
            prev = feat
        elif name.startswith("Mconv1_stage"):
            prev = torch.cat([heads[(stage - 1, 1)], heads[(stage - 1, 2)], feat], 1)
        got = nchw(acts[name])
        if L["ksize"] == 0:
            want = F.max_pool2d(prev, 2, 2)
            assert torch.equal(got, want), name
            n_pool += 1
        else:
            w = ref.params[f"{L['module']}.{name}.weight"].half().double()
            b = ref.params[f"{L['module']}.{name}.bias"].double()
            pre = F.conv2d(prev, w, b, padding=L["ksize"] // 2)
            mag = F.conv2d(prev.abs(), w.abs(), b.abs(), padding=L["ksize"] // 2)
            want = pre.clamp_min(0) if L["relu"] else pre
            KC.within_limit(got, want, mag, L["ksize"] ** 2 * L["Cin"] + net.splits[name] + 1, rounded=[pre], what=f"layerwise: {name}")
            n_conv += 1
        prev = got
        if name == "conv4_4_CPM":
            feat = got
        if name.startswith("conv5_5_CPM") or name.startswith("Mconv7_stage"):
            heads[(stage, int(name[-1]))] = got
    return n_conv, n_pool


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


# d0 = rel-L2(ref16s, ref32) per input size and output, weights `random:openpose` seed 0, input net_input(B, H, W); produced by
#     python -m tests.openpose_cases
D0 = {
    (1, 40, 56): (1.3179e-03, 1.3140e-03),
    (2, 64, 88): (1.4722e-03, 1.6382e-03),
    (1, 184, 184): (1.7337e-03, 1.7240e-03),
}


def references(B, H, W):
    ref = RefBodyPose(OP.random_state_dict(0))
    x = net_input(B, H, W)
    with torch.no_grad():
        p32, h32 = ref.forward(x, "fp32")
        p16, h16 = ref.forward(x, "fp16s")
    return x, (p32, h32), (p16, h16)


def check_end_to_end(paf, heat, B, H, W):
    """measured against the oracle, never against the kernel: rel-L2(product, ref32) <= 1.5 d0 (two independent sets of roundings add
    in quadrature, sqrt 2, plus slack) and rel-L2(product, ref16s) <= d0 (the product is nearer its own regime than that regime is to fp32)"""
    _, r32, r16 = references(B, H, W)
    d0 = D0[(B, H, W)]
    for name, got, a32, a16, d in (("paf", paf, r32[0], r16[0], d0[0]), ("heat", heat, r32[1], r16[1], d0[1])):
        e32, e16 = rel_l2(got, a32), rel_l2(got, a16)
        print(f"END2END {(B, H, W)} {name}: vs fp32 {e32:.3e} (limit {1.5 * d:.3e}), vs fp16s {e16:.3e} (limit {d:.3e})")
        assert e32 <= 1.5 * d, (name, e32, d)
        assert e16 <= d, (name, e16, d)


# ---------------------------------------------------------------- planted skeletons
# one person in a local frame (x, y), parts in OpenPose order: nose neck Rsho Relb Rwri Lsho Lelb Lwri Rhip Rkne Rank Lhip Lkne Lank Reye Leye Rear Lear
PERSON = [(20, 8), (20, 18), (10, 18), (6, 30), (4, 42), (30, 18), (34, 30), (36, 42), (14, 40), (13, 52), (12, 64), (26, 40), (27, 52),
          (28, 64), (17, 5), (23, 5), (13, 7), (27, 7)]
CANVAS = (96, 128)
ORIGINS = [(16, 16), (72, 16)]
MISSING = (1, 4)                                   # person 1 lacks its right wrist
THIRD = {1: (64, 22), 2: (64, 44), 3: (64, 66)}    # neck, right shoulder, right elbow of a "person" of three joints


def planted_people():
    """-> list of {part index: (x, y)}: two people (joints of one part >= 16 px apart and >= 16 px from every border) and the stub"""
    people = []
    for n, (ox, oy) in enumerate(ORIGINS):
        people.append({i: (ox + x, oy + y) for i, (x, y) in enumerate(PERSON) if (n, i) != MISSING})
    people.append(dict(THIRD))
    return people


def planted_maps(people=None, sigma=2.0, band=1.5):
    """heat [H, W, 19]: a Gaussian blob (peak 1.0) per joint; paf [H, W, 38]: the limb's unit vector inside a 3-px band around it"""
    people = planted_people() if people is None else people
    H, W = CANVAS
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    heat, paf = np.zeros((H, W, 19)), np.zeros((H, W, 38))
    for person in people:
        for i, (x, y) in person.items():
            heat[:, :, i] = np.maximum(heat[:, :, i], np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / (2 * sigma ** 2)))
        for k, (a, b) in enumerate(OP.LIMB_SEQ):
            if a - 1 not in person or b - 1 not in person:
                continue
            (xa, ya), (xb, yb) = person[a - 1], person[b - 1]
            d = np.array([xb - xa, yb - ya], np.float64)
            n = np.linalg.norm(d)
            u = d / n
            t = np.clip(((xx - xa) * u[0] + (yy - ya) * u[1]), 0, n)
            dist = np.sqrt((xx - xa - t * u[0]) ** 2 + (yy - ya - t * u[1]) ** 2)
            cx, cy = [c - 19 for c in OP.MAP_IDX[k]]
            paf[:, :, cx][dist <= band] = u[0]
            paf[:, :, cy][dist <= band] = u[1]
    return heat, paf


def noise_photo(H=64, W=88, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


if __name__ == "__main__":
    torch.set_num_threads(16)
    for size in ((1, 40, 56), (2, 64, 88), (1, 184, 184)):
        _, r32, r16 = references(*size)
        print(f"    {size}: ({rel_l2(r16[0], r32[0]):.4e}, {rel_l2(r16[1], r32[1]):.4e}),")
