"""Per-kernel parity cases shared by the CPU (host-emulated kernels, small shapes) and GPU (-m gpu, real
gfx950 library, real site shapes) test modules.  Every case compares a C-ABI entry point with the same
operation written in plain torch fp32 on the SAME fp16-rounded inputs; tolerances are stated per case
(fp16 output rounding is 2^-11 = 4.9e-4 relative).  The GEMM, convolution and weight-gradient cases compare with fp64 references
computed on the CPU and add an elementwise limit derived from the arithmetic (within_limit) to their norm-wise ones."""
import functools
import math

import os

import torch
import torch.nn.functional as F

from controllora_amd import kernels as K

f16, f32 = torch.float16, torch.float32


# every main-loop variant the tile sweeps of the two kernel test files run (a literal: a tile the library gains is added here on purpose)
ALL_TILE_CFGS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 21, 22, 23, 26, 31, 32, 33, 41, 42, 43, 51, 52, 53, 54, 55, 56, 57, 58, 59]


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-20))


def no_outliers(out, ref, what=""):
    """elementwise guard beside the rel-L2 checks: a handful of wrong elements in a large tensor (a race that corrupts a few
    rows of a few tiles -- seen on hardware with an epilogue variant in round 3) moves rel-L2 by 1e-4..1e-3 only and would
    pass a norm-wise limit; no element may be further from the reference than a few fp16 ulps of the largest value."""
    out, ref = out.detach().float().cpu(), ref.detach().float().cpu()
    lim = 6e-3 * max(1.0, float(ref.abs().max()))
    worst = float((out - ref).abs().max())
    assert worst < lim, f"{what}: {int(((out - ref).abs() >= lim).sum())} elements off by up to {worst:.3f} (limit {lim:.3f})"


def rnd(shape, dev, gen, scale=1.0, dtype=f16):
    return (torch.randn(shape, generator=gen) * scale).to(dtype).to(dev)


U16 = 2.0 ** -11 * (1 + 2.0 ** -10)      # one fp16 rounding, relative to the magnitude rounded, second-order term included
U32 = 2.0 ** -23                         # one fp32 accumulation step, relative to sum |a_i| |b_i| (2^-23, not 2^-24: covers a truncating accumulator)
SUB16 = 2.0 ** -25                       # half a unit of the fp16 subnormal range: the floor of an fp16 rounding
MAX_AUTO_SPLIT = 16                      # the most slabs plan_gemm chooses on its own (split_k = 0)


def d64(t):
    """the fp64 references live on the CPU, whatever device the kernels ran on"""
    return t.detach().double().cpu()


def fp16_round(t):
    """the `.half().float()` of a reference formula, on an fp64 tensor"""
    return t.half().double()


def within_limit(out, ref, mag, L, rounded=None, ops=(), what=""):
    """The elementwise limit beside the norm-wise ones.  rel-L2 < 6e-4 is blind to single elements (0.05 added to ONE output of a
    300 x 72 GEMM moves rel from 2.1e-4 to 5.5e-4; at 16384 x 320 one element may be off by 1.0); no_outliers allows every
    element 6e-3 of the largest value.  Here every element gets its own limit, DERIVED from the arithmetic the kernel performs -- never
    measured from the kernel's output:

      * every fp16 rounding of a value x contributes 2^-11 |x| (1 + 2^-10) (half a unit in the last place, plus the second-order term:
        the value rounded differs from the reference by the other errors), and at least 2^-25 (fp16 subnormals).  `rounded` lists
        the fp64 values rounded; default: the output itself, once.  A reference formula that has `.half().float()` in the middle
        names that intermediate value too (the kernel may round there or may not: either way it is within one rounding of it);
      * an fp32 accumulation of L terms contributes L 2^-23 sum_i |a_i| |b_i|: `mag` is that sum in fp64 -- |A| @ |B|^T for a GEMM,
        F.conv2d / its autograd on absolute inputs and weights for a convolution -- and the products of two fp16 values are exact in
        fp32.  2^-23 and not 2^-24 covers an accumulator that truncates; split-K adds its number of slabs to L (their fp32 sum);
      * every fp32 operand the fused epilogue adds (bias, row add, adapter term, residual before the rounding) is one more term:
        `ops` = [(|operand| in fp64, how many fp32 operations it takes)] adds to both `mag` and L;
      * an fp32 output (the weight gradients) has no fp16 term: rounded=(), limit = M 2^-23 (|dY|^T |X|).

    For K beyond a few thousand L 2^-23 dominates and the limit is loose: the norm-wise assertions stay beside it.  Fails with the
    count and the worst offender, like no_outliers; returns the worst error / limit ratio and prints it with the family of `what`."""
    out = d64(out)
    ref, mag = ref.reshape(out.shape), mag.reshape(out.shape)
    assert ref.dtype == torch.float64 and mag.dtype == torch.float64
    for a, n in ops:
        mag, L = mag + a.reshape(out.shape), L + n
    lim = L * U32 * mag
    for r_ in ([ref] if rounded is None else rounded):
        lim = lim + (U16 * r_.reshape(out.shape).abs()).clamp_min(SUB16)
    err = (out - ref).abs()
    frac = torch.where(err <= lim, err / lim, torch.full_like(err, float("inf")))      # NaN compares false: an unwritten element fails
    worst = float(frac.max())
    print(f"LIMIT {what.split(':')[0]} {worst:.3f}")          # (pytest -s: the figures quoted in the case docstrings)
    if worst > 1.0:
        i = int(frac.argmax())
        at = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), out.shape))
        e_, l_ = float(err.reshape(-1)[i]), float(lim.reshape(-1)[i])
        raise AssertionError(f"{what}: {int((frac > 1.0).sum())} of {out.numel()} elements past the derived limit; worst at {at}: "
                             f"{float(out.reshape(-1)[i]):.6g} against {float(ref.reshape(-1)[i]):.6g}, off by {e_:.3g} = {e_ / l_:.1f} x its limit {l_:.3g}")
    return worst


def conv_refs64(x, w, dy, fwd, need_dx=True, need_dw=True):
    """fp64 on the CPU: y = fwd(x, w) and, by autograd, the gradients of <y, dy> with respect to x and w.  Called on the operands for
    the reference and on their absolute values for the magnitudes sum |a_i| |b_i| of within_limit (zero padding and nearest-neighbour
    upsampling keep absolute values absolute)."""
    x64, w64 = d64(x).requires_grad_(need_dx and dy is not None), d64(w).requires_grad_(need_dw and dy is not None)
    y = fwd(x64, w64)
    if x64.requires_grad or w64.requires_grad:
        y.backward(d64(dy))
    return y.detach(), x64.grad, w64.grad


def nhwc(t):
    """[B, C, H, W] -> the [B * H * W, C] matrix the kernels read and write"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def nan_out(M, N, dev):
    """an output that starts as NaN: an element a launch skips cannot hide in a reused allocation that held the right answer"""
    return torch.full((M, N), float("nan"), dtype=f16, device=dev)


@functools.lru_cache(maxsize=4)
def _gemm_problem(M, N, K_, seed):
    """operands (on the CPU), fp64 reference and magnitude of a plain GEMM: computed once per shape, shared by the tile sweeps"""
    g = torch.Generator().manual_seed(seed)
    A, B = rnd((M, K_), "cpu", g), rnd((N, K_), "cpu", g, 1 / math.sqrt(K_))
    return A, B, A.double() @ B.double().T, A.double().abs() @ B.double().abs().T


def case_gemm_plain(dev, M, N, K_, split_k=1, seed=0, tile_cfg=0):
    """fp64 A . B^T on the same fp16 operands: norm-wise 6e-4 and the derived elementwise limit (one fp16 rounding of the output, an
    fp32 sum of K + split_k terms).  The output starts as NaN.  Worst error / limit, measured: emulator 0.98, MI355X 0.96 (the
    tile_cfg 59 loop of tests/test_kernels_gpu.py: 0.83) -- with short K the final rounding alone reaches 1 / (1 + 2^-10) of the limit
    on some element of a large output."""
    A, B, ref, mag = _gemm_problem(M, N, K_, seed)
    A, B = A.to(dev), B.to(dev)
    out = K.gemm(A, B, M, N, K_, split_k=split_k, tile_cfg=tile_cfg, out=nan_out(M, N, dev))
    assert rel(out, ref) < 6e-4
    within_limit(out, ref, mag, K_ + (split_k or MAX_AUTO_SPLIT), what=f"gemm_plain: {(M, N, K_, split_k, tile_cfg)}")
    return out, ref, mag


@functools.lru_cache(maxsize=2)
def _gemm_epilogue_problem(M, N, K_):
    g = torch.Generator().manual_seed(1)
    A, B = rnd((M, K_), "cpu", g), rnd((N, K_), "cpu", g, 1 / math.sqrt(K_))
    bias, rowadd, res = rnd((N,), "cpu", g, dtype=f32), rnd((4, N), "cpu", g), rnd((M, N), "cpu", g)
    T, U = rnd((M, 8), "cpu", g, dtype=f32), rnd((N, 4), "cpu", g, dtype=f32)
    seg = (torch.arange(N) // (N // 2)).tolist()
    T64, U64 = T.double(), U.double()
    lora = torch.stack([T64[:, s * 4:(s + 1) * 4] @ U64[n] for n, s in enumerate(seg)], 1)
    lora_mag = torch.stack([T64[:, s * 4:(s + 1) * 4].abs() @ U64[n].abs() for n, s in enumerate(seg)], 1)
    ra = rowadd.double().repeat_interleave(M // 4, 0)
    pre = A.double() @ B.double().T + bias.double() + ra + 0.7 * lora
    ref = fp16_round(pre) + res.double()
    mag = A.double().abs() @ B.double().abs().T
    ops = [(bias.double().abs().expand(M, N), 1), (ra.abs(), 1), (0.7 * lora_mag, 6), (res.double().abs(), 1)]
    return (A, B, bias, rowadd, res, T, U), pre, ref, mag, ops


def case_gemm_epilogue(dev, M=200, N=96, K_=64, split_k=1, tile_cfg=0):
    """bias + row add + two-segment rank-4 adapter + residual.  The reference formula rounds before the residual and the output is
    rounded again: two fp16 roundings in the derived limit, four fp32 epilogue operands (the adapter term: four products, their sum,
    the scale).  Worst error / limit, measured: emulator 0.88, MI355X 0.84."""
    ins, pre, ref, mag, ops = _gemm_epilogue_problem(M, N, K_)
    A, B, bias, rowadd, res, T, U = (t.to(dev) for t in ins)
    out = K.gemm(A, B, M, N, K_, bias=bias, rowadd=rowadd, rows_per_batch=M // 4, residual=res, lora_t=T, lora_u=U,
                 lora_seg=N // 2, lora_scale=0.7, split_k=split_k, tile_cfg=tile_cfg)
    assert rel(out, ref) < 6e-4
    within_limit(out, ref, mag, K_ + (split_k or MAX_AUTO_SPLIT), rounded=[pre, ref], ops=ops, what=f"gemm_epilogue: {(M, N, K_, split_k, tile_cfg)}")


@functools.lru_cache(maxsize=3)
def _no_rowadd_problem(M, N, K_):
    g = torch.Generator().manual_seed(41)
    A, B = rnd((M, K_), "cpu", g), rnd((N, K_), "cpu", g, 1 / math.sqrt(K_))
    bias, res = rnd((N,), "cpu", g, dtype=f32), rnd((M, N), "cpu", g)
    nseg = 2 if N % 32 == 0 else 1                     # lora_seg must be a multiple of 16
    seg_w = N // nseg
    T, U = rnd((M, 4 * nseg), "cpu", g, dtype=f32), rnd((N, 4), "cpu", g, dtype=f32)
    Ut = rnd((4, N), "cpu", g, dtype=f32)                                                                # dgrad form: u(n, j) = Ut[j, n]
    seg = (torch.arange(N) // seg_w).tolist()
    T64, U64 = T.double(), U.double()
    ref = dict(base=A.double() @ B.double().T, mag=A.double().abs() @ B.double().abs().T, bias=bias.double().expand(M, N), res=res.double(),
               lora=torch.stack([T64[:, s_ * 4:(s_ + 1) * 4] @ U64[n] for n, s_ in enumerate(seg)], 1),
               lora_mag=torch.stack([T64[:, s_ * 4:(s_ + 1) * 4].abs() @ U64[n].abs() for n, s_ in enumerate(seg)], 1),
               lora_tr=T64[:, :4] @ Ut.double(), lora_tr_mag=T64[:, :4].abs() @ Ut.double().abs())
    return (A, B, bias, res, T, U, Ut), seg_w, ref


def case_gemm_epilogue_no_rowadd(dev, M=300, N=320, K_=128, tile_cfg=0, split_k=1):
    """The epilogue shapes of the attention / transformer projections (no time-embedding row add): the 8-wave tiles take
    their two-phase chunk loop here (all T rows / residual chunks requested before the first is used) -- (a) bias + rank-4
    adapter + residual, N split in two adapter segments; (b) the transposed-U form of the dgrad launches; (c) bias +
    residual without an adapter; (d) no operands at all.  Ragged M (rows past the matrix re-read the tile's first row).
    Every output: norm-wise 6e-4, the fixed no_outliers limit and the derived elementwise limit (within_limit; fp64 references).
    Worst error / limit, measured: emulator 0.89, MI355X 0.89."""
    ins, seg_w, r = _no_rowadd_problem(M, N, K_)
    A, B, bias, res, T, U, Ut = (t.to(dev) for t in ins)
    base, L = r["base"], K_ + (split_k or MAX_AUTO_SPLIT)
    o_bias, o_res = (r["bias"].abs(), 1), (r["res"].abs(), 1)
    kw = dict(split_k=split_k, tile_cfg=tile_cfg)
    tag = f"gemm_epilogue_no_rowadd: {(M, N, K_, split_k, tile_cfg)} "

    def check(out, pre, ops, what, residual=True, outliers=True):
        want = fp16_round(pre) + r["res"] if residual else fp16_round(pre)
        assert rel(out, want) < 6e-4
        if outliers:
            no_outliers(out, want, what)
        within_limit(out, want, r["mag"], L, rounded=[pre, want], ops=ops + ([o_res] if residual else []), what=tag + what)

    out = K.gemm(A, B, M, N, K_, bias=bias, residual=res, lora_t=T, lora_u=U, lora_seg=seg_w, lora_scale=0.7, **kw)
    check(out, base + r["bias"] + 0.7 * r["lora"], [o_bias, (0.7 * r["lora_mag"], 6)], "bias + adapter + residual")
    again = K.gemm(A, B, M, N, K_, bias=bias, residual=res, lora_t=T, lora_u=U, lora_seg=seg_w, lora_scale=0.7, **kw)
    assert torch.equal(out, again), "the same launch twice must give the same bits"
    out = K.gemm(A, B, M, N, K_, lora_t=T, lora_u=U, lora_seg=seg_w, lora_scale=1.0, **kw)            # no bias, no residual
    check(out, base + r["lora"], [(r["lora_mag"], 6)], "adapter only", residual=False)
    out = K.gemm(A, B, M, N, K_, residual=res, lora_t=T[:, :4].contiguous(), lora_u=Ut, lora_seg=N, lora_u_tr=True, lora_r=4, **kw)
    check(out, base + r["lora_tr"], [(r["lora_tr_mag"], 6)], "transposed-U adapter + residual")
    again = K.gemm(A, B, M, N, K_, residual=res, lora_t=T[:, :4].contiguous(), lora_u=Ut, lora_seg=N, lora_u_tr=True, lora_r=4, **kw)
    assert torch.equal(out, again), "the same launch twice must give the same bits"
    out = K.gemm(A, B, M, N, K_, bias=bias, residual=res, **kw)
    check(out, base + r["bias"], [o_bias], "bias + residual")
    out = K.gemm(A, B, M, N, K_, residual=res, **kw)
    check(out, base, [], "residual only", outliers=False)


def case_gemm_fused_down(dev, M=150, N=320, K_=128, nseg=1, tile_cfg=0, u_tr=False, t_in_rows=None, bias=True, residual=True):
    """clora_epilogue_t.lora_dpack: the rank-4 adapter down-projection T = A . D^T evaluated inside the projection GEMM
    (reference models.py:232-282: `attn.to_x(h) + scale * to_x_lora(h)`).  Checks (a) the T the launch WRITES against fp64
    A . D^T (+ the precomputed part) and against the stand-alone clora_lora_down kernel, (b) the GEMM output against the
    unfused formula, elementwise, (c) bit-identical repeat launches.  t_in_rows: None = no precomputed part, 0 = one row per GEMM
    row, > 0 = broadcast rows (control batch 1).  nseg column segments of N / nseg columns (a multiple of 320)."""
    from controllora_amd import ops
    g = torch.Generator().manual_seed(43)
    A, B = rnd((M, K_), dev, g), rnd((N, K_), dev, g, 1 / math.sqrt(K_))
    bias_t = rnd((N,), dev, g, dtype=f32) if bias else None
    res = rnd((M, N), dev, g) if residual else None
    seg_w = N // nseg
    Ds = [rnd((4, K_), dev, g, 1 / math.sqrt(K_), dtype=f32) for _ in range(nseg)]
    if u_tr:
        assert nseg == 1
        U = rnd((4, N), dev, g, dtype=f32)
    else:
        U = rnd((N, 4), dev, g, dtype=f32)
    t_in, mask = None, 0
    if t_in_rows is not None:
        rows = t_in_rows or M
        t_in = rnd((rows, 4 * nseg), dev, g, dtype=f32)
        mask = 1                                                  # segment 0 only (the q adapter)
    T_ref = torch.cat([A.double() @ D.double().T for D in Ds], 1)
    if t_in is not None:
        T_ref[:, :4] += (t_in.double().repeat(M // rows, 1) if rows != M else t_in.double())[:, :4]
    pack = ops.ADAPTER_PACKS.get(Ds)
    kw = dict(bias=bias_t, residual=res, lora_u=U, lora_seg=seg_w, lora_scale=0.7, lora_u_tr=u_tr, lora_r=4,
              split_k=1, tile_cfg=tile_cfg, _tuned=False)
    T = torch.full((M, 4 * nseg), float("nan"), dtype=f32, device=dev)
    out = K.gemm(A, B, M, N, K_, lora_t=T, lora_dpack=pack, lora_t_in=t_in, lora_t_in_mask=mask,
                 lora_t_in_rows=(t_in_rows or 0) if t_in is not None else 0, **kw)
    eT = float((T.double().cpu() - T_ref.cpu()).norm() / T_ref.norm())
    assert eT < 2e-6, f"T written by the fused launch: rel {eT:.2e}"
    T2 = torch.empty_like(T)
    for s_, D in enumerate(Ds):                                   # the stand-alone kernel computes the same quantity
        K.lora_down(A, D, T2, 4 * s_, M, K_)
    if t_in is None:
        assert rel(T, T2) < 2e-6
    seg = (torch.arange(N) // seg_w).tolist()
    Tr = T_ref.float().to(dev)
    if u_tr:
        lora = Tr @ U
    else:
        lora = torch.stack([Tr[:, s_ * 4:(s_ + 1) * 4] @ U[n] for n, s_ in enumerate(seg)], 1)
    ref = A.float() @ B.float().T + 0.7 * lora
    if bias:
        ref = ref + bias_t
    ref = ref.half().float()
    if residual:
        ref = ref + res.float()
    assert rel(out, ref) < 6e-4
    no_outliers(out, ref, "fused down-projection")
    T3 = torch.empty_like(T)
    again = K.gemm(A, B, M, N, K_, lora_t=T3, lora_dpack=pack, lora_t_in=t_in, lora_t_in_mask=mask,
                   lora_t_in_rows=(t_in_rows or 0) if t_in is not None else 0, **kw)
    assert torch.equal(out, again) and torch.equal(T, T3), "the same launch twice must give the same bits"
    # the unfused launch fed with the T the fused one wrote gives the same output bits (same epilogue arithmetic)
    kw["tile_cfg"] = K.fused_down_tile(M, seg_w, tile_cfg)       # the tile the fused launch ran on (the library's replacement rule)
    unf = K.gemm(A, B, M, N, K_, lora_t=T, **kw)
    assert rel(unf, out) < 2e-5 or torch.equal(unf, out)      # same T, same epilogue formula; the non-hoisted variants order the four products differently
    return eT


def case_rank_control(dev, Mc=300, Cc=64, C_=128, rc=4, n=3, scale=0.8, strided_grad=True):
    """ops.control_terms_rank (clora_rank_compose / _mix / _compose_bwd + the deferred weight-gradient jobs) against the formula it
    replaces, evaluated by torch autograd in fp32: c_l = s U_c,l (D_c,l ctrl), Tq_l = c_l D_q,l^T (reference models.py:214-218,
    237-238) -- outputs, d ctrl and the gradients of all three matrices of every site."""
    from controllora_amd import ops
    g = torch.Generator().manual_seed(17)
    ctrl = rnd((Mc, Cc), dev, g).requires_grad_(True)
    P = lambda *sh, sc=1.0: torch.nn.Parameter((torch.randn(sh, generator=g) * sc).to(dev))
    layers = [(P(rc, Cc, sc=Cc ** -0.5), P(C_, rc, sc=0.5), P(4, C_, sc=C_ ** -0.5)) for _ in range(n)]
    outs = ops.control_terms_rank(ctrl, layers, scale)
    # the incoming gradients: column blocks of one [Mc, 12] buffer (what lora_proj hands back for a fused q | k | v projection)
    gbuf = [torch.randn((Mc, 12), generator=g).to(dev) for _ in range(n)]
    grads = [b[:, :4] if strided_grad else b[:, :4].contiguous() for b in gbuf]
    torch.autograd.backward(outs, grads)
    K.lora_wgrad_flush()
    c32 = ctrl.detach().float().clone().requires_grad_(True)
    refp = [tuple(w.detach().clone().requires_grad_(True) for w in tri) for tri in layers]
    ref = [(scale * ((c32 @ Dc.T) @ Uc.T)) @ Dq.T for Dc, Uc, Dq in refp]
    torch.autograd.backward(ref, [b[:, :4].float() for b in gbuf])
    errs = {"Tq": max(rel(o, r_) for o, r_ in zip(outs, ref)), "dctrl": rel(ctrl.grad, c32.grad)}
    for k, idx in (("dDc", 0), ("dUc", 1), ("dDq", 2)):
        errs[k] = max(rel(layers[l][idx].grad, refp[l][idx].grad) for l in range(n))
    assert errs["Tq"] < 1e-5 and errs["dctrl"] < 1e-3 and errs["dUc"] < 1e-5 and errs["dDq"] < 1e-5 and errs["dDc"] < 5e-4, errs
    return errs


@functools.lru_cache(maxsize=4)
def _conv_problem(Bn, H, W, Ci, Co, stride, pad, ups, asym, seed):
    """operands on the CPU, fp64 references (F.conv2d and its autograd) and the magnitudes (the same on absolute values)"""
    g = torch.Generator().manual_seed(seed)
    x = rnd((Bn, Ci, H, W), "cpu", g)
    w = rnd((Co, Ci, 3, 3), "cpu", g, 1 / math.sqrt(Ci * 9))
    xin = F.interpolate(x.double(), scale_factor=2.0, mode="nearest") if ups else x.double()
    fwd = (lambda x_, w_: F.conv2d(F.pad(x_, (0, 1, 0, 1)), w_, stride=2)) if asym else (lambda x_, w_: F.conv2d(x_, w_, stride=stride, padding=pad))
    Ho, Wo = fwd(xin[:1, :1], w.double()[:1, :1]).shape[2:]
    dy = rnd((Bn, Co, Ho, Wo), "cpu", g)
    y, dx, dw = conv_refs64(xin, w, dy, fwd)
    ya, dxa, dwa = conv_refs64(xin.abs(), w.abs(), dy.abs(), fwd)
    ref = dict(y=nhwc(y), y_mag=nhwc(ya), dx=nhwc(dx), dx_mag=nhwc(dxa), dw=dw, dw_mag=dwa,
               db=dy.double().sum((0, 2, 3)), db_mag=dy.double().abs().sum((0, 2, 3)))
    return x, w, dy, (Ho, Wo), tuple(xin.shape[2:]), ref


def case_conv(dev, Bn, H, W, Ci, Co, stride=1, pad=1, ups=False, asym=False, seed=2, tile_cfg=0, kchunk=0):
    """forward, dgrad and wgrad of one 3x3 conv configuration against F.conv2d autograd in fp64.
    kchunk > 0: forward and dgrad additionally run with the channel-chunk-major K order (clora_conv_t.kchunk).
    Beside the norm-wise limits every output passes the derived elementwise limit (within_limit): forward and dgrad one fp16 rounding
    and an fp32 sum of 9 Ci (9 Co) + slabs terms, dW and db fp32 sums of M terms -- also where they are ADDED to a buffer of ones
    (conv_wgrad_into, conv_wgrad_staged: the fill is one more fp32 operand per launch).
    Worst error / limit, measured: forward / dgrad emulator 0.93, MI355X 0.93; dW / db emulator 0.16, MI355X 0.013."""
    xc, wc, dyc, (Ho, Wo), (Hi, Wi), r = _conv_problem(Bn, H, W, Ci, Co, stride, pad, ups, asym, seed)
    x, w, dy = xc.to(dev), wc.to(dev), dyc.to(dev)
    tag = f"{(Bn, H, W, Ci, Co, stride, pad, ups, asym, tile_cfg, kchunk)}"
    xn = x.permute(0, 2, 3, 1).contiguous()
    wp = w.permute(0, 2, 3, 1).contiguous().reshape(Co, 9 * Ci)
    cd, Ho2, Wo2 = K.conv_fwd_desc(H, W, Ci, 3, stride, pad, upsample=ups, asym_pad=asym)
    assert (Ho2, Wo2) == (Ho, Wo)
    M = Bn * Ho * Wo
    sk = 1 if tile_cfg else 0
    out = K.gemm(xn, wp, M, Co, 9 * Ci, conv=cd, tile_cfg=tile_cfg, split_k=sk, out=nan_out(M, Co, dev))
    assert rel(out, r["y"]) < 6e-4
    within_limit(out, r["y"], r["y_mag"], 9 * Ci + (sk or MAX_AUTO_SPLIT), what="conv: fwd " + tag)
    if kchunk:
        from controllora_amd.ops import conv_k_order
        cdk, _, _ = K.conv_fwd_desc(H, W, Ci, 3, stride, pad, upsample=ups, asym_pad=asym, kchunk=kchunk)
        for sk in (1, 2, 3):
            outk = K.gemm(xn, conv_k_order(wp.reshape(Co, 9, Ci), kchunk), M, Co, 9 * Ci, conv=cdk, tile_cfg=tile_cfg, split_k=sk)
            assert rel(outk, r["y"]) < 6e-4, (sk, rel(outk, out))
            within_limit(outk, r["y"], r["y_mag"], 9 * Ci + sk, what=f"conv: fwd kchunk split {sk} " + tag)
    wd = w.permute(1, 2, 3, 0).contiguous().reshape(Ci, 9 * Co)
    dyn = dy.permute(0, 2, 3, 1).contiguous()
    cdd = K.conv_dgrad_desc(Ho, Wo, Co, Hi, Wi, 3, 2 if asym else stride, pad, asym_pad=asym)
    skd = 2 if tile_cfg else 0
    dx = K.gemm(dyn, wd, Bn * Hi * Wi, Ci, 9 * Co, conv=cdd, tile_cfg=tile_cfg, split_k=skd, out=nan_out(Bn * Hi * Wi, Ci, dev))
    assert rel(dx, r["dx"]) < 6e-4
    within_limit(dx, r["dx"], r["dx_mag"], 9 * Co + (skd or MAX_AUTO_SPLIT), what="conv: dgrad " + tag)
    if kchunk and Co % kchunk == 0:
        from controllora_amd.ops import conv_k_order
        cddk = K.conv_dgrad_desc(Ho, Wo, Co, Hi, Wi, 3, 2 if asym else stride, pad, asym_pad=asym, kchunk=kchunk)
        dxk = K.gemm(dyn, conv_k_order(wd.reshape(Ci, 9, Co), kchunk), Bn * Hi * Wi, Ci, 9 * Co, conv=cddk, tile_cfg=tile_cfg,
                     split_k=skd)
        assert rel(dxk, r["dx"]) < 6e-4
        within_limit(dxk, r["dx"], r["dx_mag"], 9 * Co + (skd or MAX_AUTO_SPLIT), what="conv: dgrad kchunk " + tag)
    if ups:
        pooled = K.pool2x2_sum(dx.reshape(Bn, Hi * Wi, Ci), Bn, H, W, Ci)
        ref = F.avg_pool2d(r["dx"].reshape(Bn, Hi, Wi, Ci).permute(0, 3, 1, 2), 2) * 4
        assert rel(pooled, ref.permute(0, 2, 3, 1).reshape(Bn, H * W, Ci)) < 1e-3
    want_w, mag_w = nhwc(r["dw"]).reshape(Co, 9 * Ci), nhwc(r["dw_mag"]).reshape(Co, 9 * Ci)        # [Co, Ci, 3, 3] -> [Co, (ky, kx, ci)]
    dW, db = K.conv_wgrad(dyn, xn, M, Co, 9 * Ci, cd, with_bias=True)
    assert rel(dW, want_w) < 1e-4
    assert rel(db, r["db"]) < 1e-4
    within_limit(dW, want_w, mag_w, M, rounded=(), what="conv_dw: dW " + tag)
    within_limit(db, r["db"], r["db_mag"], M, rounded=(), what="conv_dw: db " + tag)
    dW1 = K.conv_wgrad(dyn, xn, M, Co, 9 * Ci, cd)                                                    # without the bias column
    within_limit(dW1, want_w, mag_w, M, rounded=(), what="conv_dw: dW without bias " + tag)
    assert rel(K.colsum(dyn.reshape(M, Co), M, Co), r["db"]) < 1e-4
    if Ci % 8 == 0 and not ups:
        # trainable-conv path: one pack launch for both fp16 operands, gradients accumulated into OIHW .grad buffers
        wf, wdg = K.conv_weight_pack(w.float().contiguous(), Ci, True)
        assert torch.equal(wf, wp) and torch.equal(wdg, wd)
        gW = torch.ones((Co, Ci, 3, 3), dtype=f32, device=dev)
        gb = torch.ones((Co,), dtype=f32, device=dev)
        one_w, one_b = (torch.ones_like(r["dw"]), 1), (torch.ones_like(r["db"]), 1)
        K.conv_wgrad_into(dyn, xn, M, Co, 9 * Ci, cd, gW, gb)
        assert rel(gW - 1, r["dw"]) < 1e-4 and rel(gb - 1, r["db"]) < 1e-4
        within_limit(gW, r["dw"] + 1, r["dw_mag"], M, rounded=(), ops=[one_w], what="conv_dw: into gW " + tag)
        within_limit(gb, r["db"] + 1, r["db_mag"], M, rounded=(), ops=[one_b], what="conv_dw: into gb " + tag)
        stage = torch.zeros(Co * 9 * Ci + Co, dtype=f32, device=dev)          # persistent staging + unpack (the product path)
        gW.fill_(1.0), gb.fill_(1.0)
        for rep in (1, 2):
            K.conv_wgrad_staged(dyn, xn, M, Co, 9 * Ci, cd, stage, gW, gb, Ci)
            assert rel(gW - 1, rep * r["dw"]) < 1e-4 and rel(gb - 1, rep * r["db"]) < 1e-4
            assert float(stage.abs().max()) == 0.0
            within_limit(gW, rep * r["dw"] + 1, rep * r["dw_mag"], rep * M, rounded=(), ops=[one_w], what="conv_dw: staged gW " + tag)
            within_limit(gb, rep * r["db"] + 1, rep * r["db_mag"], rep * M, rounded=(), ops=[one_b], what="conv_dw: staged gb " + tag)


@functools.lru_cache(maxsize=2)
def _wgrad_patch_problem(Bn, H, W, Ci, Co, seed, stride):
    g = torch.Generator().manual_seed(seed)
    x = rnd((Bn, Ci, H, W), "cpu", g)
    w = rnd((Co, Ci, 3, 3), "cpu", g, 1 / math.sqrt(9 * Ci))
    Ho, Wo = (H, W) if stride == 1 else (H // 2, W // 2)              # stride 2: the downsamplers' F.pad(0, 1, 0, 1) + stride 2 (H, W even)
    dy = rnd((Bn, Co, Ho, Wo), "cpu", g)
    fwd = (lambda x_, w_: F.conv2d(x_, w_, padding=1)) if stride == 1 else (lambda x_, w_: F.conv2d(F.pad(x_, (0, 1, 0, 1)), w_, stride=2))
    _, _, dw = conv_refs64(x, w, dy, fwd, need_dx=False)
    _, _, dwa = conv_refs64(x.abs(), w.abs(), dy.abs(), fwd, need_dx=False)
    return x, dy, nhwc(dw).reshape(Co, 9 * Ci), nhwc(dwa).reshape(Co, 9 * Ci), dy.double().sum((0, 2, 3)), dy.double().abs().sum((0, 2, 3))


def case_conv_wgrad_patch(dev, Bn, H, W, Ci, Co, seed=21, stride=1):
    """Round 6 (conv_wgrad_patch_kernel): the weight / bias gradient of a large-map 3x3 stride-1 pad-1 convolution with 32 or 64 input
    channels (the hint encoder's 512^2 / 256^2 / 128^2 stages, reference models.py:470-543 ConvBlock2D / SimpleDownEncoderBlock2D under
    loss.backward(), train...:786) on the patch-staged kernel vs fp64 torch autograd, and vs the gather kernel it replaces there
    ("wgrad_patch" 0) -- same products, another summation order (fp32 atomics in both).  Both kernels' dW and db also pass the derived
    elementwise limit M 2^-23 (|dY|^T |X|) (within_limit).  Worst error / limit, measured: emulator 0.016, MI355X 0.004."""
    xc, dyc, want_w, mag_w, want_b, mag_b = _wgrad_patch_problem(Bn, H, W, Ci, Co, seed, stride)
    x, dy = xc.to(dev), dyc.to(dev)
    Ho, Wo = dy.shape[2:]
    tag = f"conv_wgrad_patch: {(Bn, H, W, Ci, Co, stride)} "
    xn = x.permute(0, 2, 3, 1).contiguous().reshape(-1, Ci)
    dyn = dy.permute(0, 2, 3, 1).contiguous().reshape(-1, Co)
    cd, Ho2, Wo2 = K.conv_fwd_desc(H, W, Ci, 3, stride, 1 if stride == 1 else 0, asym_pad=stride == 2)
    assert (Ho2, Wo2) == (Ho, Wo)
    M = Bn * Ho * Wo
    dW, db = K.conv_wgrad(dyn, xn, M, Co, 9 * Ci, cd, with_bias=True)
    assert rel(dW, want_w) < 1e-4 and rel(db, want_b) < 1e-4, (rel(dW, want_w), rel(db, want_b))
    no_outliers(dW, want_w, "conv_wgrad_patch dW")
    within_limit(dW, want_w, mag_w, M, rounded=(), what=tag + "dW")
    within_limit(db, want_b, mag_b, M, rounded=(), what=tag + "db")
    K.set_option("wgrad_patch", 0)
    try:
        dW0, db0 = K.conv_wgrad(dyn, xn, M, Co, 9 * Ci, cd, with_bias=True)
    finally:
        K.set_option("wgrad_patch", int(os.environ.get("CLORA_WGRAD_PATCH", "1")))
    assert rel(dW, dW0) < 2e-5 and rel(db, db0) < 2e-5
    within_limit(dW0, want_w, mag_w, M, rounded=(), what=tag + "gather dW")
    within_limit(db0, want_b, mag_b, M, rounded=(), what=tag + "gather db")
    dW2 = K.conv_wgrad(dyn, xn, M, Co, 9 * Ci, cd)                      # without the bias gradient
    assert rel(dW2, want_w) < 1e-4
    within_limit(dW2, want_w, mag_w, M, rounded=(), what=tag + "dW without bias")


@functools.lru_cache(maxsize=2)
def _strip_problem(Bn, H, W, Ci, Co, seed):
    g = torch.Generator().manual_seed(seed)
    x = rnd((Bn, Ci, H, W), "cpu", g)
    w = rnd((Co, Ci, 3, 3), "cpu", g, 1 / math.sqrt(9 * Ci))
    bias = rnd((Co,), "cpu", g, dtype=f32)
    dy = rnd((Bn, Co, H, W), "cpu", g)
    fwd = lambda x_, w_: F.conv2d(x_, w_, padding=1)
    y, dx, _ = conv_refs64(x, w, dy, fwd, need_dw=False)
    ya, dxa, _ = conv_refs64(x.abs(), w.abs(), dy.abs(), fwd, need_dw=False)
    res = rnd((Bn * H * W, Co), "cpu", g)
    return x, w, bias, dy, res, nhwc(y), nhwc(ya), nhwc(dx), nhwc(dxa)


def case_conv_strip(dev, Bn, H, W, Ci, Co, seed=22):
    """Round 6 (conv3x3_strip_kernel, tile_cfg 61): forward (+ bias) and dgrad of a large-map 3x3 stride-1 pad-1 convolution with 32 / 64
    channels (the hint encoder's 512^2 / 256^2 stages, reference models.py:470-543) through the default launch path -- kernels.gemm picks
    the strip kernel where clora_conv_strip_eligible says so -- vs fp64 torch, and vs the implicit GEMM it replaces there.
    A block walks rows_per_block = max(8, ceil(H * strips / strip_blocks)) rows (launch_strip; strip_blocks = 512), capped at H: every
    H <= 8 is ONE row chunk per strip.  H = 17 gives three chunks of 8, 8 and 1 rows: in the second and third the halo row above y_beg
    belongs to the neighbouring chunk (not to the zero padding), the last chunk is a single row, and the row staged past a chunk's end
    (`live ? y : y_beg`) is a real row of the next chunk that must not be used.
    Forward (bias: one fp32 operand), the implicit GEMM and the dgrad also pass the derived elementwise limit (within_limit).
    Worst error / limit, measured: emulator 0.97, MI355X 0.97."""
    import ctypes
    from controllora_amd import capi
    xc, wc, bc, dyc, resc, y, y_mag, wantd, dx_mag = _strip_problem(Bn, H, W, Ci, Co, seed)
    x, w, bias, dy, res = xc.to(dev), wc.to(dev), bc.to(dev), dyc.to(dev), resc.to(dev)
    tag = f"conv_strip: {(Bn, H, W, Ci, Co)} "
    xn = x.permute(0, 2, 3, 1).contiguous().reshape(-1, Ci)
    wp = w.permute(0, 2, 3, 1).contiguous().reshape(Co, 9 * Ci)
    cd, _, _ = K.conv_fwd_desc(H, W, Ci, 3, 1, 1)
    M = Bn * H * W
    lib = capi.lib().cdll
    assert lib.clora_conv_strip_eligible(M, Co, ctypes.byref(cd)) == 1
    want = y + bc.double()
    o_bias = (bc.double().abs().expand(M, Co), 1)
    out = K.gemm(xn, wp, M, Co, 9 * Ci, conv=cd, bias=bias, out=nan_out(M, Co, dev))
    assert rel(out, want) < 6e-4, rel(out, want)
    no_outliers(out, want, "conv_strip fwd")
    within_limit(out, want, y_mag, 9 * Ci, ops=[o_bias], what=tag + "fwd")
    ref = K.gemm(xn, wp, M, Co, 9 * Ci, conv=cd, bias=bias, tile_cfg=2, split_k=1)         # the implicit GEMM on the same operands
    assert rel(out, ref) < 3e-4
    within_limit(ref, want, y_mag, 9 * Ci + 1, ops=[o_bias], what=tag + "implicit GEMM")
    assert torch.equal(out, K.gemm(xn, wp, M, Co, 9 * Ci, conv=cd, bias=bias))             # bit-stable
    wd = w.permute(1, 2, 3, 0).contiguous().reshape(Ci, 9 * Co)
    dyn = dy.permute(0, 2, 3, 1).contiguous().reshape(-1, Co)
    cdd = K.conv_dgrad_desc(H, W, Co, H, W, 3, 1, 1)
    if lib.clora_conv_strip_eligible(M, Ci, ctypes.byref(cdd)) == 1:
        dx = K.gemm(dyn, wd, M, Ci, 9 * Co, conv=cdd, out=nan_out(M, Ci, dev))
        assert rel(dx, wantd) < 6e-4, rel(dx, wantd)
        no_outliers(dx, wantd, "conv_strip dgrad")
        within_limit(dx, wantd, dx_mag, 9 * Co, what=tag + "dgrad")
    # a launch the strip kernel cannot take (residual in the epilogue) falls back to the library's own choice under tile_cfg 61
    fb = K.gemm(xn, wp, M, Co, 9 * Ci, conv=cd, bias=bias, residual=res, tile_cfg=61, split_k=1)
    assert rel(fb, want + resc.double()) < 6e-4
    within_limit(fb, want + resc.double(), y_mag, 9 * Ci + 1, ops=[o_bias, (resc.double().abs(), 1)], what=tag + "fallback with residual")


@functools.lru_cache(maxsize=2)
def _patch_ups_problem(Bn, H, W, Ci, Co, seed):
    g = torch.Generator().manual_seed(seed)
    x = rnd((Bn, Ci, H, W), "cpu", g)
    w = rnd((Co, Ci, 3, 3), "cpu", g, 1 / math.sqrt(Ci * 9))
    fwd = lambda x_, w_: F.conv2d(F.interpolate(x_, scale_factor=2.0, mode="nearest"), w_, padding=1)
    return x, w, nhwc(conv_refs64(x, w, None, fwd)[0]), nhwc(conv_refs64(x.abs(), w.abs(), None, fwd)[0])


def case_conv_patch_upsampled(dev, Bn, H, W, Ci, Co, tile_cfg, seed=13):
    """conv3x3_patch_kernel on conv(nearest-2x(x)) (Upsample2D): the patch lives at the output resolution; fp64 reference, norm-wise
    and derived elementwise limit.  Worst error / limit, measured: see case_conv_patch."""
    from controllora_amd.ops import conv_k_order
    xc, wc, yref, y_mag = _patch_ups_problem(Bn, H, W, Ci, Co, seed)
    x, w = xc.to(dev), wc.to(dev)
    M = Bn * 4 * H * W
    xn = x.permute(0, 2, 3, 1).contiguous().reshape(Bn * H * W, Ci)
    wp = conv_k_order(w.permute(0, 2, 3, 1).contiguous().reshape(Co, 9, Ci), 64)
    cd, Ho, Wo = K.conv_fwd_desc(H, W, Ci, 3, 1, 1, upsample=True, kchunk=64)
    assert (Ho, Wo) == (2 * H, 2 * W) and K.conv_patch_eligible(M, cd, tile_cfg)
    for sk in (1, 2):
        out = K.gemm(xn, wp, M, Co, 9 * Ci, conv=cd, tile_cfg=tile_cfg, split_k=sk, out=nan_out(M, Co, dev))
        assert rel(out, yref) < 6e-4, (sk, rel(out, yref))
        within_limit(out, yref, y_mag, 9 * Ci + sk, what=f"conv_patch: upsampled {(Bn, H, W, Ci, Co, tile_cfg, sk)}")


@functools.lru_cache(maxsize=2)
def _patch_problem(Bn, H, W, Ci, Co, seed, backward):
    g = torch.Generator().manual_seed(seed)
    x = rnd((Bn, Ci, H, W), "cpu", g)
    w = rnd((Co, Ci, 3, 3), "cpu", g, 1 / math.sqrt(Ci * 9))
    dy = rnd((Bn, Co, H, W), "cpu", g)
    bias = rnd((Co,), "cpu", g, dtype=f32)
    res = rnd((Bn * H * W, Co), "cpu", g)
    fwd = lambda x_, w_: F.conv2d(x_, w_, padding=1)
    y, dx, _ = conv_refs64(x, w, dy if backward else None, fwd, need_dw=False)
    ya, dxa, _ = conv_refs64(x.abs(), w.abs(), dy.abs() if backward else None, fwd, need_dw=False)
    return x, w, dy, bias, res, nhwc(y), nhwc(ya), nhwc(dx) if backward else None, nhwc(dxa) if backward else None


def case_conv_patch(dev, Bn, H, W, Ci, Co, tile_cfg, seed=12, fwd_only=False):
    """conv3x3_patch_kernel (tile_cfg 71..75): forward and dgrad of a stride-1 pad-1 conv with the slab-major K order,
    split-K 1..3, bias + residual epilogue, against F.conv2d autograd in fp64 -- and the shape must really take the patch path.
    Norm-wise 6e-4 and the derived elementwise limit (within_limit) on every output.
    Worst error / limit, measured: emulator 0.69, MI355X 0.62."""
    from controllora_amd.ops import conv_k_order
    backward = Co % 64 == 0 and not fwd_only
    xc, wc, dyc, bc, resc, yref, y_mag, dxref, dx_mag = _patch_problem(Bn, H, W, Ci, Co, seed, backward)
    x, w, dy, bias, res = xc.to(dev), wc.to(dev), dyc.to(dev), bc.to(dev), resc.to(dev)
    tag = f"conv_patch: {(Bn, H, W, Ci, Co, tile_cfg)} "
    M = Bn * H * W
    xn = x.permute(0, 2, 3, 1).contiguous().reshape(M, Ci)
    wp = conv_k_order(w.permute(0, 2, 3, 1).contiguous().reshape(Co, 9, Ci), 64)
    cd, _, _ = K.conv_fwd_desc(H, W, Ci, 3, 1, 1, kchunk=64)
    assert K.conv_patch_eligible(M, cd, tile_cfg), "shape does not take the patch kernel"
    for sk in (1, 2, 3):
        out = K.gemm(xn, wp, M, Co, 9 * Ci, conv=cd, tile_cfg=tile_cfg, split_k=sk, out=nan_out(M, Co, dev))
        assert rel(out, yref) < 6e-4, (sk, rel(out, yref))
        within_limit(out, yref, y_mag, 9 * Ci + sk, what=tag + f"fwd split {sk}")
    out = K.gemm(xn, wp, M, Co, 9 * Ci, conv=cd, tile_cfg=tile_cfg, split_k=1, bias=bias, residual=res)
    pre = yref + bc.double()
    assert rel(out, pre + resc.double()) < 6e-4
    within_limit(out, pre + resc.double(), y_mag, 9 * Ci + 1, ops=[(bc.double().abs().expand(M, Co), 1), (resc.double().abs(), 1)],
                 what=tag + "bias + residual")            # the sum is formed in fp32 and rounded once (clora_epilogue.h CLORA_RES_ADD)
    out = K.gemm(xn, wp, M, Co, 9 * Ci, conv=cd, _tuned=False)                 # the library's own choice for an untuned shape
    assert rel(out, yref) < 6e-4
    within_limit(out, yref, y_mag, 9 * Ci + MAX_AUTO_SPLIT, what=tag + "library's choice")
    if backward:
        wd = conv_k_order(w.permute(1, 2, 3, 0).contiguous().reshape(Ci, 9, Co), 64)
        dyn = dy.permute(0, 2, 3, 1).contiguous().reshape(M, Co)
        cdd = K.conv_dgrad_desc(H, W, Co, H, W, 3, 1, 1, kchunk=64)
        assert K.conv_patch_eligible(M, cdd, tile_cfg)
        for sk in (1, 2):
            dx = K.gemm(dyn, wd, M, Ci, 9 * Co, conv=cdd, tile_cfg=tile_cfg, split_k=sk, out=nan_out(M, Ci, dev))
            assert rel(dx, dxref) < 6e-4, (sk,)
            within_limit(dx, dxref, dx_mag, 9 * Co + sk, what=tag + f"dgrad split {sk}")


PACK_CAP = 2048 * 256          # elements one trip of the capped grids of conv_weight_pack_kernel / conv_wgrad_unpack_kernel covers
PACK_MULTI_CAP = 1024 * 256    # the same for their multi-job forms (clora_ew.hip: 1024 blocks per job)


def case_conv_pack_unpack_past_cap(dev, shapes=((232, 256, 256),), seed=85):
    """conv_weight_pack_kernel and conv_wgrad_unpack_kernel where their grid is capped (2048 blocks of 256) and the grid-stride loop
    takes a second trip: Co * 9 * Cip > 524,288 for the first (Co, Ci, Cip) of `shapes`.  No convolution runs: the entry points are
    called directly on random data.  Pack: fp32 weights that fp16 cannot represent -> both operands equal the permuted, ROUNDED
    weight bit for bit (padded input channels Cip > Ci and padded output channels Cop > Co are zero); the outputs start as NaN.
    Unpack: a random staging buffer is ADDED to non-zero grad_w / grad_b -- equal to the permuted fp32 sum bit for bit -- and the
    staging buffer is left zero.  The multi-job forms (clora_conv_weight_pack_multi_f32 / clora_conv_wgrad_unpack_multi_f32: grid.x =
    the largest job's, capped at 1024 blocks, the smaller jobs' surplus blocks idle) run all `shapes` in ONE launch and give the same."""
    g = torch.Generator().manual_seed(seed)
    assert shapes[0][0] * 9 * shapes[0][2] > PACK_CAP > PACK_MULTI_CAP
    probs = []
    for Co, Ci, Cip in shapes:
        Cop = (Co + 7) // 8 * 8
        w = (torch.randn((Co, Ci, 3, 3), generator=g) * 1.0009765625 + 1e-5).to(dev)          # not representable in fp16: the cast has to round
        wh = torch.zeros((Cop, Cip, 3, 3), dtype=f16, device=dev)
        wh[:Co, :Ci] = w.half()
        want_f = wh[:Co].permute(0, 2, 3, 1).reshape(Co, 9 * Cip)                          # [co][tap][ci]
        want_d = wh.permute(1, 2, 3, 0).reshape(Cip, 9 * Cop)                              # [ci][tap][co]
        stage = rnd((Co * 9 * Cip + Co,), dev, g, dtype=f32)
        gw, gb = rnd((Co, Ci, 3, 3), dev, g, dtype=f32), rnd((Co,), dev, g, dtype=f32)
        add_w = stage[:Co * 9 * Cip].reshape(Co, 3, 3, Cip)[..., :Ci].permute(0, 3, 1, 2)
        probs.append((Co, Ci, Cip, Cop, w, want_f, want_d, stage, gw, gb, gw + add_w, gb + stage[Co * 9 * Cip:]))

    def check_pack(fwd, dgrad, want_f, want_d, what):
        assert torch.equal(fwd, want_f), (what, "fwd", int((fwd != want_f).sum()), "elements differ")
        if dgrad is not None:
            assert torch.equal(dgrad, want_d), (what, "dgrad", int((dgrad != want_d).sum()), "elements differ")

    def check_unpack(st, nw, gw, gb, want_w, want_b, with_bias, what):
        assert torch.equal(gw, want_w), (what, "grad_w", int((gw != want_w).sum()), "elements differ")
        assert float(st[:nw].abs().max()) == 0.0, (what, "staging buffer not left zero")
        if with_bias:
            assert torch.equal(gb, want_b), (what, "grad_b", int((gb != want_b).sum()), "elements differ")
            assert float(st[nw:].abs().max()) == 0.0, (what, "bias staging not left zero")

    nanh = lambda *sh: torch.full(sh, float("nan"), dtype=f16, device=dev)
    pack_jobs, unpack_jobs, keep = [], [], []
    for Co, Ci, Cip, Cop, w, want_f, want_d, stage, gw, gb, want_w, want_b in probs:
        what = f"{(Co, Ci, Cip)}"
        for need_dgrad in (True, False):
            fwd, dgrad = K.conv_weight_pack(w, Cip, need_dgrad, out=(nanh(Co, 9 * Cip), nanh(Cip, 9 * Cop) if need_dgrad else None))
            check_pack(fwd, dgrad, want_f, want_d, "pack " + what)
        for with_bias in (True, False):
            st, w_, b_ = stage.clone(), gw.clone(), gb.clone()
            nw = Co * 9 * Cip
            K._call("clora_conv_wgrad_unpack_f32", K.ptr(st[:nw]), K.ptr(st[nw:]) if with_bias else None, K.ptr(w_),
                    K.ptr(b_) if with_bias else None, Co, Ci, 3, Cip)
            check_unpack(st, nw, w_, b_, want_w, want_b, with_bias, "unpack " + what)
            assert with_bias or torch.equal(st[nw:], stage[nw:])                           # no bias gradient: the bias block is not touched
        outs = (nanh(Co, 9 * Cip), nanh(Cip, 9 * Cop), stage.clone(), gw.clone(), gb.clone())
        keep.append(outs)
        pack_jobs.append(K.conv_pack_job(w, Cip, outs[0], outs[1]))
        unpack_jobs.append(K.conv_unpack_job(outs[2], outs[3], outs[4], Cip))
    K.conv_weight_pack_multi(pack_jobs)
    K.conv_wgrad_unpack_multi(unpack_jobs)
    for (Co, Ci, Cip, Cop, w, want_f, want_d, stage, gw, gb, want_w, want_b), (fwd, dgrad, st, w_, b_) in zip(probs, keep):
        check_pack(fwd, dgrad, want_f, want_d, f"multi-job pack {(Co, Ci, Cip)}")
        check_unpack(st, Co * 9 * Cip, w_, b_, want_w, want_b, True, f"multi-job unpack {(Co, Ci, Cip)}")


def case_tile_order(dev, tile_cfg, order, seed=21):
    """the tile -> XCD assignment permutes which workgroup computes which tile and nothing else: plain GEMM with split-K and the
    adapter epilogue, and a 3x3 conv (patch kernel for tile_cfg 71..76), give the same bits under every order"""
    from controllora_amd.ops import conv_k_order
    g = torch.Generator().manual_seed(seed)
    M, N, K_ = 600, 336, 192                       # several tiles each way, ragged edges (N % 16 == 0 for the adapter epilogue)
    if order == "grid":                            # whole divisors each way for every tile shape up to 256 x 256: the rectangle assignment applies
        M, N = 1024, 512
    A, B = rnd((M, K_), dev, g), rnd((N, K_), dev, g, 1 / math.sqrt(K_))
    bias, res = rnd((N,), dev, g, dtype=f32), rnd((M, N), dev, g)
    T, U = rnd((M, 4), dev, g, dtype=f32), rnd((N, 4), dev, g, dtype=f32)
    Bn, H, W, Ci, Co = (8, 8, 8, 128, 256) if order == "grid" else (4, 8, 8, 128, 136)
    x = rnd((Bn * H * W, Ci), dev, g)
    w = conv_k_order(rnd((Co, 9, Ci), dev, g, 1 / math.sqrt(Ci * 9)), 64)
    cd, _, _ = K.conv_fwd_desc(H, W, Ci, 3, 1, 1, kchunk=64)
    patch = tile_cfg >= 71

    def run():
        outs = []
        if not patch:
            for sk in ((1, 2, 3) if order == "grid" else (1, 3)):
                outs.append(K.gemm(A, B, M, N, K_, split_k=sk, tile_cfg=tile_cfg))
            outs.append(K.gemm(A, B, M, N, K_, bias=bias, residual=res, lora_t=T, lora_u=U, lora_scale=0.5, split_k=1, tile_cfg=tile_cfg))
        for sk in (1, 2):
            outs.append(K.gemm(x, w, Bn * H * W, Co, 9 * Ci, conv=cd, tile_cfg=tile_cfg, split_k=sk))
        return outs

    try:
        K.set_tile_order("m")
        base = run()
        K.set_tile_order(order)
        other = run()
    finally:
        K.set_tile_order(K.DEFAULT_TILE_ORDER)
    assert rel(base[0], A.float() @ B.float().T) < 6e-4 if not patch else True
    for a, b in zip(base, other):
        assert torch.equal(a, b)


def case_conv_padded_channels(dev, seed=9):
    """3 -> padded 8 input channels (the hint encoder's conv_in): packing pads with zeros, the OIHW gradient drops them"""
    g = torch.Generator().manual_seed(seed)
    Bn, H, W, Ci, Cip, Co = 2, 8, 8, 3, 8, 16
    x = rnd((Bn, Ci, H, W), dev, g)
    w = rnd((Co, Ci, 3, 3), dev, g, dtype=f32)
    xin = x.float().clone()
    w32 = w.half().float().clone().requires_grad_(True)
    y = F.conv2d(xin, w32, padding=1)
    dy = rnd((Bn, Co, H, W), dev, g)
    y.backward(dy.float())
    xn = torch.zeros((Bn, H, W, Cip), dtype=f16, device=dev)
    xn[..., :Ci] = x.permute(0, 2, 3, 1)
    wf, _ = K.conv_weight_pack(w, Cip, False)
    cd, Ho, Wo = K.conv_fwd_desc(H, W, Cip, 3, 1, 1)
    M = Bn * Ho * Wo
    out = K.gemm(xn.reshape(M, Cip), wf, M, Co, 9 * Cip, conv=cd)
    assert rel(out, y.detach().permute(0, 2, 3, 1).reshape(M, Co)) < 1e-3
    gW = torch.zeros((Co, Ci, 3, 3), dtype=f32, device=dev)
    dyn = dy.permute(0, 2, 3, 1).contiguous().reshape(M, Co)
    K.conv_wgrad_into(dyn, xn.reshape(M, Cip), M, Co, 9 * Cip, cd, gW, None)
    assert rel(gW, w32.grad) < 1e-4
    stage = torch.zeros(Co * 9 * Cip + Co, dtype=f32, device=dev)
    K.conv_wgrad_staged(dyn, xn.reshape(M, Cip), M, Co, 9 * Cip, cd, stage, gW, None, Cip)
    assert rel(gW, 2 * w32.grad) < 1e-4 and float(stage.abs().max()) == 0.0


def _attn_ref(q, k, v, H, scale):
    B, Nq, HD = q.shape
    D = HD // H
    qh = q.float().reshape(B, Nq, H, D).permute(0, 2, 1, 3)
    kh = k.float().reshape(B, -1, H, D).permute(0, 2, 1, 3)
    vh = v.float().reshape(B, -1, H, D).permute(0, 2, 1, 3)
    p = torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1)
    return (p @ vh).permute(0, 2, 1, 3).reshape(B, Nq, HD)


def case_attention(dev, B, H, Nq, Nk, D, seed=3, fused_qkv=False, tol=2e-3, ramp=0.0):
    """ramp > 0: keys grow along the sequence (k_j scaled by 1 + ramp*j/Nk) and q is 3x larger, so the row maxima keep
    rising from KV tile to KV tile by more than the forward kernel's lazy-rescale threshold: the rebase path runs on
    later tiles too, for some queries of a wave and not for others."""
    g = torch.Generator().manual_seed(seed)
    scale = D ** -0.5
    if fused_qkv:   # q,k,v are column slices of one [B*N, 3*H*D] buffer (self-attention layout)
        qkv = rnd((B * Nq, 3 * H * D), dev, g)
        q2, k2, v2 = qkv[:, :H * D], qkv[:, H * D:2 * H * D], qkv[:, 2 * H * D:]
    else:
        q2, k2, v2 = rnd((B * Nq, H * D), dev, g), rnd((B * Nk, H * D), dev, g), rnd((B * Nk, H * D), dev, g)
    if ramp > 0:
        assert not fused_qkv
        w = 1.0 + ramp * torch.arange(Nk, dtype=f32).repeat(B)[:, None] / Nk
        k2 = (k2.float().cpu() * w).to(f16).to(dev)
        q2 = (q2.float() * 3.0).to(f16)
    q3 = q2.reshape(B, Nq, H * D).float().clone().requires_grad_(True)
    k3 = k2.reshape(B, Nk, H * D).float().clone().requires_grad_(True)
    v3 = v2.reshape(B, Nk, H * D).float().clone().requires_grad_(True)
    ref = _attn_ref(q3, k3, v3, H, scale)
    o, lse = K.attn_fwd(q2, k2, v2, B, H, Nq, Nk, D, scale)
    assert rel(o, ref.detach().reshape(B * Nq, H * D)) < tol, rel(o, ref.detach().reshape(B * Nq, H * D))
    dO = rnd((B * Nq, H * D), dev, g)
    ref.backward(dO.reshape(B, Nq, H * D).float())
    dq, dk, dv = torch.empty_like(q2.contiguous()), torch.empty_like(k2.contiguous()), torch.empty_like(v2.contiguous())
    K.attn_bwd(q2, k2, v2, o, dO, lse, B, H, Nq, Nk, D, scale, dq, dk, dv)
    for name, a, b_ in (("dq", dq, q3.grad), ("dk", dk, k3.grad), ("dv", dv, v3.grad)):
        e = rel(a, b_.reshape(a.shape))
        assert e < 2 * tol, (name, e)


def case_attention_negative_logits(dev, B, H, Nq, Nk, D, seed=31):
    """every logit of the FIRST KV tile far below -88 (q = +8, k = -8 on every channel: logit
    -64 * sqrt(D)): the lazy exponent reference must not rescale the still-empty accumulators by exp2(+huge) = inf
    (0 * inf = NaN).  Later tiles carry ordinary keys, so the result is an ordinary softmax over those."""
    g = torch.Generator().manual_seed(seed)
    scale = D ** -0.5
    q2 = torch.full((B * Nq, H * D), 8.0, dtype=f16, device=dev)
    k2 = rnd((B * Nk, H * D), dev, g, scale=0.05)
    v2 = rnd((B * Nk, H * D), dev, g)
    k3 = k2.reshape(B, Nk, H * D).clone()
    k3[:, :min(64, Nk)] = -8.0                               # the whole first tile (or every key when Nk <= 64)
    k2 = k3.reshape(B * Nk, H * D).contiguous()
    ref = _attn_ref(q2.reshape(B, Nq, H * D), k2.reshape(B, Nk, H * D), v2.reshape(B, Nk, H * D), H, scale)
    o, lse = K.attn_fwd(q2, k2, v2, B, H, Nq, Nk, D, scale)
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(lse).all())
    e = rel(o, ref.reshape(B * Nq, H * D))
    assert e < 2e-3, e
    dO = rnd((B * Nq, H * D), dev, g)
    dq, dk, dv = torch.empty_like(q2), torch.empty_like(k2), torch.empty_like(v2)
    K.attn_bwd(q2, k2, v2, o, dO, lse, B, H, Nq, Nk, D, scale, dq, dk, dv)
    for name, t_ in (("dq", dq), ("dk", dk), ("dv", dv)):
        assert bool(torch.isfinite(t_.float()).all()), (name, "a NaN / inf was computed")


def case_attention_block_order(dev, B, H, Nq, Nk, D, seed=23):
    """whole heads per XCD (tile_order != "m") only permutes which workgroup handles which (head, block): the forward
    output, LSE and the three gradients are bit-identical; the grid (3 x 6 blocks at Nq = 300, B*H = 6) is not a multiple of 8"""
    g = torch.Generator().manual_seed(seed)
    scale = D ** -0.5
    q2, k2, v2 = rnd((B * Nq, H * D), dev, g), rnd((B * Nk, H * D), dev, g), rnd((B * Nk, H * D), dev, g)
    dO = rnd((B * Nq, H * D), dev, g)

    def run():
        o, lse = K.attn_fwd(q2, k2, v2, B, H, Nq, Nk, D, scale)
        dq, dk, dv = torch.empty_like(q2), torch.empty_like(k2), torch.empty_like(v2)
        K.attn_bwd(q2, k2, v2, o, dO, lse, B, H, Nq, Nk, D, scale, dq, dk, dv)
        return o, lse, dq, dk, dv

    try:
        K.set_tile_order("m")
        base = run()
        K.set_tile_order("auto")
        other = run()
    finally:
        K.set_tile_order(K.DEFAULT_TILE_ORDER)
    for a, b_ in zip(base, other):
        assert torch.equal(a, b_)


def case_groupnorm(dev, B, HW, C, G, silu, eps=1e-5, seed=4, train_params=False):
    g = torch.Generator().manual_seed(seed)
    x = (rnd((B, HW, C), dev, g).float() * 1.5 + 0.3).half()
    gamma, beta = (1 + 0.2 * rnd((C,), dev, g, dtype=f32)), 0.2 * rnd((C,), dev, g, dtype=f32)
    x32 = x.float().clone().requires_grad_(True)
    g32, b32 = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = F.group_norm(x32.permute(0, 2, 1), G, g32, b32, eps).permute(0, 2, 1)
    if silu:
        y = F.silu(y)
    out, stats = K.groupnorm_fwd(x, gamma, beta, G, eps, silu)
    assert rel(out, y.detach()) < 8e-4
    dy = rnd((B, HW, C), dev, g)
    y.backward(dy.float())
    dx, dg, db = K.groupnorm_bwd(x, dy, gamma, beta, stats, G, silu, want_param_grads=train_params)
    assert rel(dx, x32.grad) < 2e-3
    if train_params:
        assert rel(dg, g32.grad) < 1e-3 and rel(db, b32.grad) < 1e-3
    # fused second gradient (residual branch) and in-place accumulation of the affine gradients
    dres = rnd((B, HW, C), dev, g)
    acc_g, acc_b = torch.ones(C, dtype=f32, device=dev), torch.ones(C, dtype=f32, device=dev)
    dx2, _, _ = K.groupnorm_bwd(x, dy, gamma, beta, stats, G, silu, grads_into=(acc_g, acc_b) if train_params else None, dres=dres)
    assert rel(dx2, x32.grad + dres.float()) < 2e-3
    if train_params:
        assert rel(acc_g - 1, g32.grad) < 1e-3 and rel(acc_b - 1, b32.grad) < 1e-3
    else:
        # the one-launch (register-resident) passes against the two-launch scheme on the same inputs: same arithmetic, a different
        # summation order -- a few fp16 ulps on a handful of elements at most; shapes the one-launch plan does not take run the
        # same kernels twice
        K.set_option("gn_resident", 0)
        try:
            out0, stats0 = K.groupnorm_fwd(x, gamma, beta, G, eps, silu)
            dx0, _, _ = K.groupnorm_bwd(x, dy, gamma, beta, stats0, G, silu, dres=dres)
        finally:
            K.set_option("gn_resident", int(os.environ.get("CLORA_GN_RESIDENT", "1")))
        assert rel(out, out0) < 2e-4 and rel(stats, stats0) < 1e-5 and rel(dx2, dx0) < 3e-4
        out1, stats1 = K.groupnorm_fwd(x, gamma, beta, G, eps, silu)             # bit-stable
        assert torch.equal(out1, out) and torch.equal(stats1, stats)
        # the team kernels of the large maps (one launch, in-launch exchange of the partial sums) against the scheme they replace;
        # repeated calls walk the exchange epochs of the persistent state: bit-stable, and no exchange ever gave up
        K.set_option("gn_team", 0)
        try:
            out_t0, stats_t0 = K.groupnorm_fwd(x, gamma, beta, G, eps, silu)
            dx_t0, _, _ = K.groupnorm_bwd(x, dy, gamma, beta, stats_t0, G, silu, dres=dres)
        finally:
            K.set_option("gn_team", int(os.environ.get("CLORA_GN_TEAM", "2")))
        assert rel(out, out_t0) < 2e-4 and rel(stats, stats_t0) < 1e-5 and rel(dx2, dx_t0) < 3e-4
        for _ in range(2):
            dx3, _, _ = K.groupnorm_bwd(x, dy, gamma, beta, stats, G, silu, dres=dres)
            assert torch.equal(dx3, dx2)
        assert K.gn_team_errors(x.device) == 0


def case_groupnorm_concat(dev, B, HW, Ca, Cb, G, silu, eps=1e-5, seed=11):
    """Round 6 (include/clora.h clora_groupnorm_*_ex, x2 / dx2): GroupNorm over the channel concatenation of two tensors read in
    place == GroupNorm over the materialised concatenation, BIT for bit (same loads, same arithmetic, same order): output, statistics,
    the concatenated copy the kernel writes, and the backward's two gradient tensors."""
    g = torch.Generator().manual_seed(seed)
    a = (rnd((B, HW, Ca), dev, g).float() * 1.5 + 0.3).half()
    b = (rnd((B, HW, Cb), dev, g).float() * 0.7 - 0.2).half()
    C_ = Ca + Cb
    gamma, beta = (1 + 0.2 * rnd((C_,), dev, g, dtype=f32)), 0.2 * rnd((C_,), dev, g, dtype=f32)
    xc = torch.cat([a, b], -1).contiguous()
    y0, st0 = K.groupnorm_fwd(xc, gamma, beta, G, eps, silu)
    y1, st1, xcat = K.groupnorm_fwd(a, gamma, beta, G, eps, silu, x2=b)
    assert torch.equal(xcat, xc) and torch.equal(y0, y1) and torch.equal(st0, st1)
    dy, dres = rnd((B, HW, C_), dev, g), rnd((B, HW, C_), dev, g)
    for dr in (None, dres):
        dx0, _, _ = K.groupnorm_bwd(xc, dy, gamma, beta, st0, G, silu, dres=dr)
        (da, db), _, _ = K.groupnorm_bwd(xc, dy, gamma, beta, st0, G, silu, dres=dr, split_at=Ca)
        assert da.shape == (B, HW, Ca) and db.shape == (B, HW, Cb) and da.is_contiguous() and db.is_contiguous()
        assert torch.equal(da, dx0[..., :Ca]) and torch.equal(db, dx0[..., Ca:])


def case_deferred_finish(dev, B, HW, C, Kd, G, split, silu=True, seed=12, lora=False):
    """both settings of the "defer_max_rows" knob: the default (fold only in the few-rows-per-thread GroupNorm plans, finish first
    elsewhere) and 16 (fold wherever a folding kernel exists, incl. the LayerNorm backward) -- bit-identical either way"""
    for rows in (16, int(os.environ.get("CLORA_DEFER_MAX_ROWS", "4"))):
        K.set_option("defer_max_rows", rows)
        try:
            _case_deferred_finish(dev, B, HW, C, Kd, G, split, silu, seed, lora)
        finally:
            K.set_option("defer_max_rows", int(os.environ.get("CLORA_DEFER_MAX_ROWS", "4")))


def _case_deferred_finish(dev, B, HW, C, Kd, G, split, silu=True, seed=12, lora=False):
    """Round 6 (clora_deferred_t): a split-K GEMM whose finish pass is left to the GroupNorm / LayerNorm launch that reads its output
    == the same GEMM with its own finish pass followed by the plain norm launch, BIT for bit -- forward GroupNorm (the finished
    tensor must also land in the GEMM's C), GroupNorm backward and LayerNorm backward with the GEMM producing dy; epilogue = bias +
    row add + residual (+ a rank-4 adapter term for the LayerNorm case, what the attention projections' dgrad carries)."""
    g = torch.Generator().manual_seed(seed)
    M = B * HW
    A = rnd((M, Kd), dev, g)
    Wt = (rnd((C, Kd), dev, g).float() * 0.1).half()
    bias = rnd((C,), dev, g, dtype=f32)
    res = rnd((M, C), dev, g)
    rowadd = rnd((B, C), dev, g)
    gamma, beta = (1 + 0.2 * rnd((C,), dev, g, dtype=f32)), 0.2 * rnd((C,), dev, g, dtype=f32)
    kw = dict(bias=bias, residual=res, rowadd=rowadd, rows_per_batch=HW, split_k=split)
    if lora:
        kw.update(lora_t=rnd((M, 8), dev, g, dtype=f32), lora_u=rnd((8, C), dev, g, dtype=f32), lora_seg=C, lora_u_tr=True, lora_r=8)
    assert not K._PENDING
    ref = K.gemm(A, Wt, M, C, Kd, **kw)
    y0, st0 = K.groupnorm_fwd(ref.reshape(B, HW, C), gamma, beta, G, 1e-5, silu)
    out = K.gemm(A, Wt, M, C, Kd, defer=True, **kw)
    deferred = bool(K._PENDING)
    assert deferred == (split > 1 and K.DEFER_FINISH)
    y1, st1 = K.groupnorm_fwd(out.reshape(B, HW, C), gamma, beta, G, 1e-5, silu)
    assert not K._PENDING and torch.equal(out, ref) and torch.equal(y0, y1) and torch.equal(st0, st1)
    x = rnd((B, HW, C), dev, g)
    dres = rnd((B, HW, C), dev, g)
    _, stx = K.groupnorm_fwd(x, gamma, beta, G, 1e-5, silu)
    dx0, _, _ = K.groupnorm_bwd(x, ref.reshape(B, HW, C), gamma, beta, stx, G, silu, dres=dres)
    dyd = K.gemm(A, Wt, M, C, Kd, defer=True, **kw)
    dx1, _, _ = K.groupnorm_bwd(x, dyd.reshape(B, HW, C), gamma, beta, stx, G, silu, dres=dres)
    assert not K._PENDING and torch.equal(dx0, dx1)
    if C <= 1536:
        x2 = x.reshape(M, C)
        l0 = K.layernorm_bwd(x2, ref, gamma, 1e-5, dres=dres.reshape(M, C))
        dyd = K.gemm(A, Wt, M, C, Kd, defer=True, **kw)
        l1 = K.layernorm_bwd(x2, dyd, gamma, 1e-5, dres=dres.reshape(M, C))
        assert not K._PENDING and torch.equal(l0, l1)
    # the safety net: any OTHER kernel call first finishes what is pending
    dyd = K.gemm(A, Wt, M, C, Kd, defer=True, **kw)
    z = K.add(dyd, dyd)
    assert not K._PENDING and torch.equal(dyd, ref) and torch.equal(z, K.add(ref, ref))


# GroupNorm instantiations that no other GPU case reaches (profiles/norm_refactor_bits.txt lists which case reaches which): the smallest
# shape that gn_resident_plan / gn_team_plan / gn_plan (clora_norm.hip) route there, with the knobs that take it there.
#   (what, B, HW, C, G, knobs, lo, deferred)
GN_INSTANTIATION_CASES = [
    # one group of 4096 channels: a slab wider than 2048, two column chunks per thread -- gn_fwd_partial / apply2<2, 1, false> and
    # <2, 1, true>, gn_bwd_partial / apply2<2, 1> with and without the channel partials
    ("two_launch_nj2", 1, 16, 4096, 1, {}, False, False),
    ("two_launch_nj2_lo", 1, 16, 4096, 1, {}, True, False),
    # gn_fwd_partial / apply2<1, 2, true>: the remainder under "gn_unroll"
    ("two_launch_unroll_lo", 1, 64, 320, 32, dict(gn_resident=0, gn_unroll=1), True, False),
    # a 320-channel slab (two groups of 320) does not fit 256 threads: 512 threads, 12 row lanes, 6 rows per thread --
    # gn_fwd_resident_kernel<512, 8> plain, with the remainder and folding a deferred producer
    ("resident_512_8", 1, 64, 640, 2, {}, False, False),
    ("resident_512_8_lo", 1, 64, 640, 2, {}, True, False),
    ("resident_512_8_def", 1, 64, 640, 2, dict(defer_max_rows=16), False, True),
    # 64-channel slab, 400 rows: 13 rows per thread at 256 threads forward (gn_fwd_resident_kernel<256, 16, true>), 7 at 512 threads
    # backward (gn_bwd_resident_kernel<512, 8, true>), both folding the deferred producer
    ("resident_400_rows_def", 1, 400, 64, 8, dict(defer_max_rows=16), False, True),
]


def case_groupnorm_instantiation(dev, B, HW, C, G, knobs, lo, deferred, eps=1e-5, seed=17):
    """forward (8e-4), dx with dres (2e-3) and, through the trainable-affine call, dgamma / dbeta (1e-3) against fp32 torch -- the limits
    of case_groupnorm -- and a second launch of each giving the bits of the first.  lo: the input is hi + lo (clora_groupnorm_fwd_f16_lo);
    deferred: the forward's x and the backward's dy are unfinished split-K GEMMs (bias + row add + residual) that the norm folds."""
    g = torch.Generator().manual_seed(seed)
    M, Kd = B * HW, 128
    gamma, beta = (1 + 0.2 * rnd((C,), dev, g, dtype=f32)), 0.2 * rnd((C,), dev, g, dtype=f32)
    x_lo = rnd((B, HW, C), dev, g, 1e-3) if lo else None
    dy, dres = rnd((B, HW, C), dev, g), rnd((B, HW, C), dev, g)
    A, Wt = rnd((M, Kd), dev, g), rnd((C, Kd), dev, g, 0.1)
    kw = dict(bias=rnd((C,), dev, g, dtype=f32), residual=rnd((M, C), dev, g), rowadd=rnd((B, C), dev, g), rows_per_batch=HW, split_k=2)
    assert not K._PENDING
    x = K.gemm(A, Wt, M, C, Kd, **kw).reshape(B, HW, C) if deferred else (rnd((B, HW, C), dev, g).float() * 1.5 + 0.3).half()
    producer = lambda: K.gemm(A, Wt, M, C, Kd, defer=True, **kw).reshape(B, HW, C)
    x32 = (x.float() + (x_lo.float() if lo else 0)).clone().requires_grad_(True)
    g32, b32 = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = F.silu(F.group_norm(x32.permute(0, 2, 1), G, g32, b32, eps).permute(0, 2, 1))
    rows = knobs.get("defer_max_rows")
    rest = {k_: v_ for k_, v_ in knobs.items() if k_ != "defer_max_rows"}
    if rows is not None:
        K.set_option("defer_max_rows", rows)
    try:
        with options(**rest):
            fwd = lambda: K.groupnorm_fwd(producer() if deferred else x, gamma, beta, G, eps, True, x_lo=x_lo)
            out, stats = fwd()
            out1, stats1 = fwd()
            assert not K._PENDING and torch.equal(out1, out) and torch.equal(stats1, stats)
            e_y = rel(out, y.detach())
            print(f"GN_INSTANTIATION {(B, HW, C, G)} {knobs} lo={lo} deferred={deferred} y={e_y:.2e}")
            assert e_y < 8e-4
            if lo:
                return                                           # the backward recomputes from x alone: no remainder form
            # the backward: dy = the deferred tensor where there is one (the same values as x: any fp16 tensor serves as a gradient)
            gy = x if deferred else dy
            y.backward(gy.float())
            bwd = lambda **kw_: K.groupnorm_bwd(x, producer() if deferred else gy, gamma, beta, stats, G, True, **kw_)
            dx, _, _ = bwd(dres=dres)
            dx1, _, _ = bwd(dres=dres)
            assert not K._PENDING and torch.equal(dx1, dx)
            dxp, dg, db = bwd(want_param_grads=True)
            dxp1, dg1, db1 = bwd(want_param_grads=True)
            assert torch.equal(dxp1, dxp) and torch.equal(dg1, dg) and torch.equal(db1, db)
            errs = dict(dx=rel(dx, x32.grad + dres.float()), dx_params=rel(dxp, x32.grad), dgamma=rel(dg, g32.grad), dbeta=rel(db, b32.grad))
            print(f"GN_INSTANTIATION {(B, HW, C, G)} {knobs} deferred={deferred} " + " ".join(f"{k_}={v_:.2e}" for k_, v_ in errs.items()))
            assert errs["dx"] < 2e-3 and errs["dx_params"] < 2e-3 and errs["dgamma"] < 1e-3 and errs["dbeta"] < 1e-3, errs
    finally:
        if rows is not None:
            K.set_option("defer_max_rows", int(os.environ.get("CLORA_DEFER_MAX_ROWS", "4")))
    assert K.gn_team_errors(x.device) == 0


def case_gemm_fused_layernorm(dev, M, Kd, tile_cfg, seed=13, lora=False, residual=True):
    """Round 6 (clora_epilogue_t.ln_out): the LayerNorm that follows a projection, written by the projection's own launch where one
    320-column tile spans the row, == clora_layernorm_fwd_f16 on the stored output (same partition / formulas / summation order: the
    compiler may contract the final affine differently in the two kernels, so equality is asserted up to one fp16 ulp on a handful of
    elements); C itself must be bit-identical to the launch without the fused norm."""
    g = torch.Generator().manual_seed(seed)
    N = 320
    A = rnd((M, Kd), dev, g)
    Wt = (rnd((N, Kd), dev, g).float() * 0.1).half()
    bias = rnd((N,), dev, g, dtype=f32)
    res = rnd((M, N), dev, g) if residual else None
    gamma, beta = (1 + 0.2 * rnd((N,), dev, g, dtype=f32)), 0.2 * rnd((N,), dev, g, dtype=f32)
    kw = dict(bias=bias, residual=res, tile_cfg=tile_cfg, split_k=1)
    if lora:
        kw.update(lora_t=rnd((M, 4), dev, g, dtype=f32), lora_u=rnd((N, 4), dev, g, dtype=f32) * 0.1, lora_seg=N)
    ref = K.gemm(A, Wt, M, N, Kd, **kw)
    ln_ref = K.layernorm_fwd(ref, gamma, beta, 1e-5)
    slot = K.LayerNormSlot(gamma, beta, 1e-5)
    out = K.gemm(A, Wt, M, N, Kd, ln=slot, **kw)
    assert slot.out is not None, "the launch did not take the fused LayerNorm"
    assert torch.equal(out, ref)
    diff = (slot.out.float() - ln_ref.float()).abs()
    ulp = ln_ref.float().abs().clamp_min(2.0 ** -10) * 2.0 ** -10
    assert bool((diff <= ulp).all()), float((diff / ulp).max())
    assert float((diff > 0).float().mean()) < 0.02
    # a shape / tile that cannot fuse leaves the slot empty (the caller launches the norm itself)
    slot2 = K.LayerNormSlot(gamma, beta, 1e-5)
    K.gemm(A, Wt, M, N, Kd, ln=slot2, bias=bias, tile_cfg=43, split_k=1)
    assert slot2.out is None


def case_softmax_rows(dev, rows, cols, scale=0.37, seed=6):
    g = torch.Generator().manual_seed(seed)
    x = (rnd((rows, cols), dev, g).float() * 4).half()
    y = K.softmax_rows(x, scale)
    ref = torch.softmax(x.float() * scale, -1)
    assert float((y.float() - ref).abs().max()) < 1e-3 and float((y.float().sum(-1) - 1).abs().max()) < 4e-3
    K.softmax_rows(x, scale, out=x)                      # in place
    assert torch.equal(x, y)


def case_layernorm(dev, M, C, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = rnd((M, C), dev, g)
    gamma, beta = (1 + 0.2 * rnd((C,), dev, g, dtype=f32)), 0.2 * rnd((C,), dev, g, dtype=f32)
    x32 = x.float().clone().requires_grad_(True)
    y = F.layer_norm(x32, (C,), gamma, beta, 1e-5)
    assert rel(K.layernorm_fwd(x, gamma, beta, 1e-5), y.detach()) < 6e-4
    dy = rnd((M, C), dev, g)
    y.backward(dy.float())
    assert rel(K.layernorm_bwd(x, dy, gamma, 1e-5), x32.grad) < 1e-3
    dres = rnd((M, C), dev, g)                      # fused residual-branch gradient
    assert rel(K.layernorm_bwd(x, dy, gamma, 1e-5, dres=dres), x32.grad + dres.float()) < 1e-3


def case_layernorm_rows(dev, M, C, seed=25):
    """several rows in flight per wave (clora_set_option "ln_rows"): same per-row arithmetic as the one-row kernel, ragged last
    block (M not a multiple of the rows per block), forward / backward / backward with the residual-branch gradient"""
    g = torch.Generator().manual_seed(seed)
    x, dy, dres = rnd((M, C), dev, g), rnd((M, C), dev, g), rnd((M, C), dev, g)
    gamma, beta = (1 + 0.2 * rnd((C,), dev, g, dtype=f32)), 0.2 * rnd((C,), dev, g, dtype=f32)

    def run():
        return (K.layernorm_fwd(x, gamma, beta, 1e-5), K.layernorm_bwd(x, dy, gamma, 1e-5), K.layernorm_bwd(x, dy, gamma, 1e-5, dres=dres))

    try:
        K.set_option("ln_rows", 0)
        base = run()
        K.set_option("ln_rows", 1)
        rows = run()
    finally:
        K.set_option("ln_rows", 1)                                # the library default
    x32 = x.float().clone().requires_grad_(True)
    y = F.layer_norm(x32, (C,), gamma, beta, 1e-5)
    y.backward(dy.float())
    assert rel(rows[0], y.detach()) < 6e-4 and rel(rows[1], x32.grad) < 1e-3
    for a, b_ in zip(base, rows):
        assert rel(a, b_) < 1e-5, rel(a, b_)


EW_CAP = 4096 * 256        # work items (16-byte vectors, or elements for the casts) one trip of a capped elementwise grid covers (ew_grid)


def check_past_cap(out, ref, first, lim, what):
    """rel-L2 limit + no_outliers on the whole tensor and, when the launch needs more than one trip of its grid-stride loop, again on
    the part from flat index / row `first` on: a defect confined to the later trips is diluted by the first million correct vectors"""
    out, ref = out.reshape(-1, out.shape[-1]) if out.dim() > 1 else out, ref.reshape(-1, ref.shape[-1]) if ref.dim() > 1 else ref
    parts = [("", out, ref)] + ([(" past the first trip", out[first:], ref[first:])] if first < out.shape[0] else [])
    for tag, o, r_ in parts:
        e = rel(o, r_)
        assert e < lim, (what + tag, e)
        no_outliers(o, r_, what + tag)


def case_geglu(dev, M, Fdim, seed=6):
    """M * Fdim / 8 > EW_CAP: the rows from EW_CAP // (Fdim / 8) + 1 on belong to later trips of the grid-stride loop alone"""
    g = torch.Generator().manual_seed(seed)
    h = rnd((M, 2 * Fdim), dev, g)
    h32 = h.float().clone().requires_grad_(True)
    a, gg = h32.chunk(2, -1)
    y = a * F.gelu(gg)
    later = EW_CAP // (Fdim // 8) + 1
    check_past_cap(K.geglu_fwd(h), y.detach(), later, 6e-4, "geglu_fwd")
    dy = rnd((M, Fdim), dev, g)
    y.backward(dy.float())
    check_past_cap(K.geglu_bwd(h, dy), h32.grad, later, 8e-4, "geglu_bwd")


def case_lora(dev, M, Kd, N, R, x_rows=0, seed=7):
    g = torch.Generator().manual_seed(seed)
    rows = x_rows if x_rows else M
    X = rnd((rows, Kd), dev, g)
    D, U = rnd((R, Kd), dev, g, 0.3, f32), rnd((N, R), dev, g, 0.3, f32)
    T = torch.zeros((M, R + 4), dtype=f32, device=dev)
    K.lora_down(X, D, T, 4, M, Kd, x_rows=x_rows)
    Xf = X.float().repeat(M // rows, 1) if x_rows else X.float()
    Tref = Xf @ D.T
    assert rel(T[:, 4:], Tref) < 1e-5
    K.lora_down(X, D, T, 4, M, Kd, accumulate=True, x_rows=x_rows)
    assert rel(T[:, 4:], 2 * Tref) < 1e-5
    if R <= 16:                                   # second input by linearity: T = (X + X2) . D^T in one job
        X2 = rnd((M, Kd), dev, g)
        T2 = torch.zeros((M, R + 4), dtype=f32, device=dev)
        K.lora_down_multi([K.down_job(X, D, T2, 4, M, Kd, x_rows=x_rows, X2=X2)])
        assert rel(T2[:, 4:], Tref + X2.float() @ D.T) < 1e-5
    T[:, 4:] = Tref
    base = rnd((M, N), dev, g)
    nan_out = lambda: torch.full((M, N), float("nan"), dtype=f16, device=dev)      # an element the launch skips stays NaN
    y = K.lora_up(base, T, 4, U, M, N, 0.6, out=nan_out())
    ref = base.float() + (0.6 * (Tref @ U.T).half().float()).half().float()
    assert rel(y, ref) < 6e-4
    later = EW_CAP // (N // 8) + 1                # rows the capped grid of lora_up reaches on a later trip only (M * N / 8 > EW_CAP)
    if later < M:
        assert rel(y[later:], ref[later:]) < 6e-4
    y0 = K.lora_up(None, T, 4, U, M, N, 1.0, out=nan_out())
    assert rel(y0, Tref @ U.T) < 6e-4
    if later < M:
        assert rel(y0[later:], (Tref @ U.T)[later:]) < 6e-4
    # the weight gradients are ADDED to what the caller's buffer holds (the optimizer's flat gradient buffer): start from a fill
    A = rnd((rows, N), dev, g)
    fill = 0.75
    G1 = torch.full((N, R), fill, dtype=f32, device=dev)
    K.lora_wgrad(A, T, 4, G1, R, 1, M, N, R, scale=0.5, a_rows=x_rows)
    Af = A.float().repeat(M // rows, 1) if x_rows else A.float()
    assert rel(G1 - fill, 0.5 * Af.T @ Tref) < 1e-4
    G2 = torch.full((R, N), fill, dtype=f32, device=dev)
    K.lora_wgrad(A, T, 4, G2, 1, N, M, N, R, scale=1.0, a_rows=x_rows)
    assert rel(G2 - fill, (Af.T @ Tref).T) < 1e-4
    if R <= 16:                                   # reduction over fp16(A + A2)
        A2 = rnd((M, N), dev, g)
        G3 = torch.full((N, R), fill, dtype=f32, device=dev)
        K.lora_wgrad_multi([K.wgrad_job(A, T, 4, G3, R, 1, M, N, R, a_rows=x_rows, A2=A2)], dev)
        assert rel(G3 - fill, (Af + A2.float()).half().float().T @ Tref) < 1e-4


def case_lora_wgrad_multi(dev, shapes=((2113, 40), (70, 520), (300, 64)), R=4, seed=71):
    """ONE clora_lora_wgrad_multi_f16 launch whose jobs differ in M and N (grid = the largest job's: the others' surplus blocks exit;
    34 / 2 / 5 row blocks, one job with a second column block): every job's gradient equals its single-job launch bit for bit (same
    slabs, same fold order) and agrees with fp32 torch (1e-4, case_lora's limit); the buffers start from a fill."""
    g = torch.Generator().manual_seed(seed)
    fill = -0.5
    As = [rnd((M, N), dev, g) for M, N in shapes]
    Ts = [rnd((M, R), dev, g, 0.5, f32) for M, _ in shapes]
    single = [torch.full((N, R), fill, dtype=f32, device=dev) for _, N in shapes]
    multi = [s_.clone() for s_ in single]
    for A, T, G, (M, N) in zip(As, Ts, single, shapes):
        K.lora_wgrad_multi([K.wgrad_job(A, T, 0, G, R, 1, M, N, R, scale=0.5)], dev)
    K.lora_wgrad_multi([K.wgrad_job(A, T, 0, G, R, 1, M, N, R, scale=0.5) for A, T, G, (M, N) in zip(As, Ts, multi, shapes)], dev)
    for A, T, Gs, Gm, shape in zip(As, Ts, single, multi, shapes):
        assert torch.equal(Gs, Gm), (shape, "multi-job launch differs from the single-job one", rel(Gm, Gs))
        e = rel(Gm - fill, 0.5 * A.float().T @ T)
        assert e < 1e-4, (shape, e)


def case_elementwise(dev, seed=8):
    g = torch.Generator().manual_seed(seed)
    a, b = rnd((6, 40, 24), dev, g), rnd((6, 40, 24), dev, g)
    assert rel(K.add(a, b), a.float() + b.float()) < 5e-4
    assert rel(K.silu(a), F.silu(a.float())) < 5e-4
    a32 = a.float().clone().requires_grad_(True)
    F.silu(a32).backward(b.float())
    assert rel(K.silu_bwd(a, b), a32.grad) < 6e-4
    c = rnd((6, 40, 16), dev, g)
    cat = K.concat_channels(a, c)
    assert torch.equal(cat.cpu(), torch.cat([a, c], -1).cpu())
    sa, sc = K.split_channels(cat, 24)
    assert torch.equal(sa.cpu(), a.cpu()) and torch.equal(sc.cpu(), c.cpu())
    # sinusoidal timestep embedding in one launch (round 6) vs upstream's op sequence (get_timestep_embedding, flip_sin_to_cos, shift 0):
    # int64 per-sample timesteps (training), one fp32 value for the whole batch (samplers)
    half = 160
    freq = torch.exp(-math.log(10000) * torch.arange(half, dtype=f32, device=dev) / half).contiguous()
    for t, batch in ((torch.tensor([0, 999, 1, 500, 37], dtype=torch.long, device=dev), 5), (torch.tensor([981.0], dtype=f32, device=dev), 3)):
        arg = t.reshape(-1).expand(batch)[:, None].float() * freq[None, :]
        ref = torch.cat([torch.cos(arg), torch.sin(arg)], -1)
        out = K.timestep_embedding(t, batch, freq)
        assert out.shape == (batch, 2 * half) and out.dtype == f16
        assert float((out.float() - ref).abs().max()) <= 1e-3            # one fp16 rounding of a value in [-1, 1]
        frac_equal = float((out == ref.to(f16)).float().mean())
        assert frac_equal > 0.99, frac_equal


def fp16_rounding_margin(ref):
    """limit for an fp16 result checked against an fp32 reference where the project states none yet: four times the rel-L2 distance
    of the reference's own fp16 rounding from it (the error of a perfect kernel)"""
    return 4.0 * rel(ref.half(), ref)


def case_elementwise_past_cap(dev, n=(EW_CAP + 300) * 8, seed=81):
    """The elementwise kernels where their grid is capped (ew_grid: 4096 blocks of 256) and the grid-stride loop takes a second trip --
    what the product does on every activation of the upper UNet levels.  add and the two casts are one rounding of exact inputs: bit
    equality.  silu / silu_bwd keep case_elementwise's limits.  quick_gelu had no reference check: fp32 torch on the same fp16 inputs,
    limit = fp16_rounding_margin (reference rounding 2.07e-4 -> limit 8.27e-4; measured: emulator 2.07e-4, MI355X 2.07e-4).  Every
    check is repeated on the elements past the first trip alone (check_past_cap).  The entry points are called on outputs that start
    as NaN (the wrappers of kernels.py allocate theirs uninitialised, and an allocator may hand back the block that held the right
    answer a moment ago): an element a launch never writes fails the check whatever memory it landed in."""
    g = torch.Generator().manual_seed(seed)
    a, b = rnd((n,), dev, g), rnd((n,), dev, g)
    first = EW_CAP * 8                                               # 8 halves per vector

    def run(entry, *ins, dtype=f16):
        y = torch.full((n,), float("nan"), dtype=dtype, device=dev)
        K._call(entry, *[K.ptr(x, x.dtype) for x in ins], K.ptr(y), n)
        return y

    y = run("clora_add_f16", a, b)
    want = (a.float() + b.float()).half()
    assert torch.equal(y, want), ("add", int((y != want).sum()), int((y[first:] != want[first:]).sum()))
    check_past_cap(run("clora_silu_f16", a), F.silu(a.float()), first, 5e-4, "silu")
    a32 = a.float().clone().requires_grad_(True)
    F.silu(a32).backward(b.float())
    check_past_cap(run("clora_silu_bwd_f16", a, b), a32.grad, first, 6e-4, "silu_bwd")
    ref = a.float() * torch.sigmoid(1.702 * a.float())
    lim = fp16_rounding_margin(ref)
    out = run("clora_quick_gelu_f16", a)
    print(f"QUICK_GELU n={n} rel={rel(out, ref):.3e} limit={lim:.3e}")
    check_past_cap(out, ref, first, lim, "quick_gelu")
    # the casts walk ELEMENTS: n elements are 8 trips, everything from EW_CAP on is a later one
    x32 = (a.float() * 1.0009765625 + 1e-5).contiguous()             # not representable in fp16: the cast has to round
    h = run("clora_cast_f32_to_f16", x32)
    assert torch.equal(h, x32.half()), ("to_f16", int((h != x32.half()).sum()), int((h[EW_CAP:] != x32.half()[EW_CAP:]).sum()))
    back = run("clora_cast_f16_to_f32", a, dtype=f32)
    assert torch.equal(back, a.float()), ("cast_f16_to_f32", int((back != a.float()).sum()))
    for wrapped, direct in ((K.add(a, b), y), (K.quick_gelu(a), out), (K.to_f16(x32), h)):      # the wrappers launch the same thing
        assert torch.equal(wrapped, direct)


def case_copies_past_cap(dev, shape=(32, 1100), Ca=240, Cb=248, seed=82):
    """concat_channels / split_channels (clora_copy2d_f16, strided on one side) with more than EW_CAP 16-byte vectors per copy
    (35200 rows x 30 / 31 vectors): bit equality with torch.cat / slicing"""
    g = torch.Generator().manual_seed(seed)
    assert shape[0] * shape[1] * min(Ca, Cb) // 8 > EW_CAP
    a, c = rnd(shape + (Ca,), dev, g), rnd(shape + (Cb,), dev, g)
    cat = K.concat_channels(a, c)
    want = torch.cat([a, c], -1)
    assert torch.equal(cat, want), ("concat", int((cat != want).any(-1).sum()), "rows differ")
    sa, sc = K.split_channels(cat, Ca)
    assert torch.equal(sa, a) and torch.equal(sc, c), ("split", int((sa != a).any(-1).sum()), int((sc != c).any(-1).sum()), "rows differ")


def case_pool2x2_sum(dev, B, H, W, C_, seed=83):
    """clora_pool2x2_sum_f16 (backward of the nearest-neighbour 2x upsampling): dx[b, y, x] = the sum of the 2 x 2 block of dy, fp32
    torch on the same fp16 inputs.  Only case_conv(ups=True) reached it, through a convolution's dgrad and at 1e-3.  Limit =
    fp16_rounding_margin (reference rounding 2.12e-4 -> limit 8.47e-4; measured: emulator 2.12e-4, MI355X 2.12e-4), whole tensor and past the
    first trip of the capped grid (B * H * W * C / 8 > EW_CAP at the large shape)."""
    g = torch.Generator().manual_seed(seed)
    dy = rnd((B, 2 * H, 2 * W, C_), dev, g)
    d32 = dy.float()
    ref = ((d32[:, 0::2, 0::2] + d32[:, 0::2, 1::2]) + d32[:, 1::2, 0::2]) + d32[:, 1::2, 1::2]
    out = K.pool2x2_sum(dy.reshape(B, 4 * H * W, C_), B, H, W, C_)
    lim = fp16_rounding_margin(ref)
    print(f"POOL2X2 {(B, H, W, C_)} rel={rel(out, ref.reshape(B, H * W, C_)):.3e} limit={lim:.3e}")
    check_past_cap(out.reshape(-1), ref.reshape(-1), EW_CAP * 8, lim, "pool2x2_sum")


def case_colsum(dev, M, N, seed=84):
    """clora_colsum_f16 (bias gradients) against an fp64 column sum, 1e-4 as in case_conv: M > 1024 takes a second row block (fp32
    atomics join the blocks), N % 128 != 0 a ragged last column block; `out` is added to"""
    g = torch.Generator().manual_seed(seed)
    A = rnd((M, N), dev, g)
    ref = A.double().sum(0)
    assert rel(K.colsum(A, M, N), ref) < 1e-4, rel(K.colsum(A, M, N), ref)
    acc = torch.full((N,), 2.0, dtype=f32, device=dev)
    K.colsum(A, M, N, out=acc)
    assert rel(acc - 2.0, ref) < 1e-4


def case_loss_and_optimizer(dev, n=5000, seed=9):
    g = torch.Generator().manual_seed(seed)
    pred, tgt = rnd((n * 8,), dev, g), rnd((n * 8,), dev, g)
    loss = torch.zeros(1, dtype=f32, device=dev)
    dpred = torch.empty_like(pred)
    state = torch.zeros(16, dtype=f32, device=dev)
    state[3] = 1024.0
    K.mse(pred, tgt, loss, dpred, 2.0 / pred.numel(), state[3:4])
    d = pred.float() - tgt.float()
    assert abs(float(loss) / pred.numel() - float((d * d).mean())) < 1e-4
    assert rel(dpred, 1024.0 * 2.0 / pred.numel() * d) < 6e-4
    # optimizer vs torch.optim.AdamW + clip_grad_norm_ for 3 steps (one of them with an inf -> skipped)
    p0 = rnd((n,), dev, g, dtype=f32)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    pt = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([pt], lr=1e-2, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    for step in range(3):
        gr = rnd((n,), dev, g, 0.1, f32)
        scaled = gr * state[3]
        if step == 1:
            scaled = scaled.clone()
            scaled[7] = float("inf")
        K.grad_sumsq(scaled, state)
        K.optim_prep(state, 1.0, 0.9, 0.999, True, 2.0, 0.5, 2000)
        K.adamw_flat(p, scaled, m, v, state, 1e-2, 0.9, 0.999, 1e-8, 1e-2)
        if step != 1:
            pt.grad = gr.clone()
            torch.nn.utils.clip_grad_norm_([pt], 1.0)
            opt.step()
            assert float(state[3]) == (1024.0 if step == 0 else 512.0)
        else:
            assert float(state[6]) == 1.0 and float(state[3]) == 512.0
        assert rel(p, pt.detach()) < 1e-6, (step, rel(p, pt.detach()))
    assert float(state[2]) == 2.0
    # the two state slots the host writes (include/clora.h): [11] = data-parallel world size -- the flat buffer holds the SUM over two
    # ranks (2 g) and the step must land where torch's AdamW fed the mean g lands; [10] = the LR schedule's multiplier -- 0.5 against
    # torch's AdamW at half the rate.  The middle step is small enough to pass unclipped: clipped steps alone cannot tell whether the
    # divisor was applied (the clip renormalises whatever it is given), and one unclipped step alone cannot either (Adam's first update is
    # scale-free).  The unscaled norm the kernel reports in slot 9 is a sum of n fp32 squares in thread / wave / block order: 1e-5.
    for slot, value, what in ((11, 2.0, "world size 2"), (10, 0.5, "lr multiplier 0.5")):
        st = torch.zeros(16, dtype=f32, device=dev)
        st[3], st[slot] = 1024.0, value
        world, lr_mult = (value, 1.0) if slot == 11 else (1.0, value)
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        pt = torch.nn.Parameter(p0.clone())
        opt = torch.optim.AdamW([pt], lr=1e-2 * lr_mult, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
        for step, gscale in enumerate((0.1, 0.1 / math.sqrt(n), 0.1)):       # |g| ~ 0.1 sqrt(n) (clipped to 1), ~ 0.1 (not clipped), clipped
            gr = rnd((n,), dev, g, gscale, f32)
            summed = gr * (1024.0 * world)                                     # exact: powers of two
            K.grad_sumsq(summed, st)
            K.optim_prep(st, 1.0, 0.9, 0.999, True, 2.0, 0.5, 2000)
            K.adamw_flat(p, summed, m, v, st, 1e-2, 0.9, 0.999, 1e-8, 1e-2)
            pt.grad = gr.clone()
            torch.nn.utils.clip_grad_norm_([pt], 1.0)
            opt.step()
            norm = float(gr.double().norm())
            assert abs(float(st[9]) - norm) < 1e-5 * norm, (what, "norm", step, float(st[9]), norm)
            assert rel(p, pt.detach()) < 1e-6, (what, step, rel(p, pt.detach()))


def case_grad_sumsq_reproducible(dev, n=78080, graph=False, seed=93):
    """clora_grad_sumsq_f32 + clora_optim_prep_f32 on ONE gradient, ten times: sum of squares, reported norm and clip factor are the
    same BITS every time, and the norm agrees with fp64 to 1e-5 (case_loss_and_optimizer's limit).  The gradient spans six decades
    and the norm is above max_norm, so the order of the block partials shows in the last bits of the sum and the clip factor carries
    them to every parameter: with one fp32 atomic per block the norm of this very size (the DreamBooth test's flat LoRA buffer, 305
    blocks) took 2 - 4 different values in 6 launches on an MI355X, most often inside a replayed graph, and a graphed training run
    did not repeat itself.  A GEMM in front of every launch makes the blocks start unevenly.  graph (the real library only): the
    same launches captured once and replayed five times.  The emulator runs blocks one after the other: it checks the arithmetic
    and the n > 1024 blocks trip, never the ordering."""
    g = torch.Generator().manual_seed(seed)
    gr = (rnd((n,), dev, g, 1.0, f32) * torch.pow(10.0, torch.rand(n, generator=g) * 6 - 3).to(dev)).contiguous()
    A, W = rnd((1024, 64), dev, g), rnd((64, 64), dev, g)
    norm = float(gr.double().norm())
    assert norm > 10.0

    st0 = torch.zeros(16, dtype=f32, device=dev)
    st0[3] = 1.0                                                  # loss scale 1, made once: a scalar write cannot be captured

    def once():
        st = st0.clone()
        K.gemm(A, W, 1024, 64, 64)
        K.grad_sumsq(gr, st)
        sumsq = st[0:1].clone()
        K.optim_prep(st, 1.0, 0.9, 0.999, False, 2.0, 0.5, 2000)
        return sumsq, st

    first = once()
    assert abs(float(first[1][9]) - norm) < 1e-5 * norm, (float(first[1][9]), norm)
    assert float(first[1][6]) == 0.0 and 0.0 < float(first[1][5]) < 0.1          # clipped, not skipped
    runs = [once() for _ in range(9)]
    if graph:
        torch.cuda.synchronize()
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg):
            captured = once()
        for _ in range(5):
            cg.replay()
            torch.cuda.synchronize()
            runs.append((captured[0].clone(), captured[1].clone()))
    seen = sorted({(float(s_), float(st[9]), float(st[5])) for s_, st in [first] + runs})
    assert len(seen) == 1, f"{len(seen)} different (sum of squares, norm, clip factor) in {len(runs) + 1} launches on one gradient: {seen}"
    # an inf in the last block's share is counted, whatever the other blocks add
    bad = gr.clone()
    bad[n - 3] = float("inf")
    st = torch.zeros(16, dtype=f32, device=dev)
    st[3] = 1.0
    K.grad_sumsq(bad, st)
    assert float(st[1]) == 1.0
    K.optim_prep(st, 1.0, 0.9, 0.999, False, 2.0, 0.5, 2000)
    assert float(st[6]) == 1.0 and float(st[9]) == -1.0 and float(st[0]) == 0.0 and float(st[1]) == 0.0


def case_feed_forward_fused(dev, M=200, C=64, seed=12, tile_cfg=0):
    """FeedForward(GEGLU) with the activation fused into the GEMM epilogues (ops.feed_forward: GegluPack + geglu = 1 / 2)
    against (i) the unfused kernels -- bit-identical, same rounding points -- and (ii) an fp32 torch reference
    (upstream FeedForward: Linear(C, 8C) -> a * gelu_erf(g) -> Linear(4C, C), + residual), forward and d(input)."""
    from controllora_amd import ops
    g = torch.Generator().manual_seed(seed)
    Fd = 4 * C
    x = rnd((M, C), dev, g)
    w1, b1 = rnd((2 * Fd, C), dev, g, C ** -0.5), rnd((2 * Fd,), dev, g, 0.1)
    w2, b2 = rnd((C, Fd), dev, g, Fd ** -0.5), rnd((C,), dev, g, 0.1)
    res = rnd((M, C), dev, g)
    dout = rnd((M, C), dev, g)
    p1, p2 = ops.GegluPack(w1, b1), ops.LinearPack(w2, b2)
    xf = x.clone().requires_grad_(True)
    old_tuned = K._TUNING
    if tile_cfg:
        K._TUNING = {K.tuning_key(M, 2 * Fd, C, None): [tile_cfg, 1], K.tuning_key(M, Fd, C, None): [tile_cfg, 1]}
    try:
        out = ops.feed_forward(xf, p1, p2, res)
        out.backward(dout)
    finally:
        K._TUNING = old_tuned
    # (i) unfused kernels
    lp1 = ops.LinearPack(w1, b1)
    xu = x.clone().requires_grad_(True)
    out_u = ops.frozen_linear(ops.geglu(ops.frozen_linear(xu, lp1)), p2, res)
    out_u.backward(dout)
    # round 6: the fused forward forms a * gelu(g) from the fp32 accumulators and adds the residual in fp32 (ONE rounding each, the
    # unfused kernels round a, g and the branch first): the two differ by fp16 rounding, and the fused result must not be farther
    # from the fp32 reference than the unfused one (checked below); the backward reads the same stored fp16 h in both
    assert rel(out, out_u) < 6e-4, rel(out, out_u)
    assert rel(xf.grad, xu.grad) < 2e-4, rel(xf.grad, xu.grad)
    # (ii) fp32 reference
    x32 = x.float().cpu().requires_grad_(True)
    h = F.linear(x32, w1.float().cpu(), b1.float().cpu())
    a, gg = h.chunk(2, -1)
    ref = F.linear(a * F.gelu(gg), w2.float().cpu(), b2.float().cpu()) + res.float().cpu()
    ref.backward(dout.float().cpu())
    assert rel(out, ref.detach()) < 2e-3, rel(out, ref.detach())
    assert rel(out, ref.detach()) <= 1.05 * rel(out_u, ref.detach()), (rel(out, ref.detach()), rel(out_u, ref.detach()))
    assert rel(xf.grad, x32.grad) < 3e-3, rel(xf.grad, x32.grad)
    # inference: no h is written
    with torch.no_grad():
        y_inf, h_inf = K.gemm(x, p1.w, M, p1.N, p1.K, bias=p1.bias, geglu=1, geglu_keep_h=False)
        assert h_inf is None
        out_inf = ops.feed_forward(x, p1, p2, res)
    assert rel(out_inf, out.detach()) < 1e-6


def case_gemm_trunk_lo(dev, M, N, K_, split_k=1, tile_cfg=0, conv_like=False, lora=False, seed=41):
    """Round 6, compensated residual trunk (include/clora.h clora_epilogue_t.residual_lo / c_lo): inside a kernels.TrunkLo window a chain
    of three residual launches  x1 = A1 W^T + x0,  x2 = A2 W^T + x1,  x3 = A3 W^T + x2  (x0 from a launch flagged `trunk`) carries the
    rounding remainder of every sum to the next add.  Checked: hi stays ONE fp16 rounding (2.0e-4 rel-L2) away from the un-rounded fp32
    chain at every link, hi + lo reproduces the fp32 chain to fp32-accumulation accuracy (the plain chain is 3-4e-4
    away from it), the window leaves nothing registered, and outside a window the same calls give the plain results bit for bit."""
    g = torch.Generator().manual_seed(seed)
    W = rnd((N, K_), dev, g, 1 / math.sqrt(K_))
    As = [rnd((M, K_), dev, g) for _ in range(4)]
    bias = rnd((N,), dev, g, dtype=f32)
    kw = dict(split_k=split_k, tile_cfg=tile_cfg)
    if lora:
        kw.update(lora_t=rnd((M, 4), dev, g, dtype=f32), lora_u=rnd((N, 4), dev, g, 0.1, dtype=f32), lora_seg=N)
    plain = [K.gemm(As[0], W, M, N, K_, bias=bias, **kw)]
    for i in range(1, 4):
        plain.append(K.gemm(As[i], W, M, N, K_, bias=bias, residual=plain[-1], **kw))
    with K.TrunkLo(True):
        hi = [K.gemm(As[0], W, M, N, K_, bias=bias, trunk=True, **kw)]
        los = [K._TRUNK_LO[hi[0].data_ptr()][1]]
        for i in range(1, 4):
            hi.append(K.gemm(As[i], W, M, N, K_, bias=bias, residual=hi[-1].reshape(M, N), **kw))
            los.append(K._TRUNK_LO[hi[-1].data_ptr()][1])
            assert hi[-2].data_ptr() not in K._TRUNK_LO              # consumed by the add that read it
    assert not K._TRUNK_LO and not K._TRUNK_LO_ON[0]
    Wf = W.float().cpu()
    upd = None
    if lora:
        upd = (kw["lora_t"].float().cpu() @ kw["lora_u"].float().cpu().T)
    ref = torch.zeros(M, N)
    for i in range(4):
        ref = ref + As[i].float().cpu() @ Wf.T + bias.float().cpu() + (upd if upd is not None else 0)
        comp = hi[i].float().cpu() + los[i].float().cpu()
        assert rel(comp, ref) < 3e-6 * (i + 1) + 2e-6, (i, rel(comp, ref))
        assert rel(hi[i], ref) < 2.3e-4                           # hi = ONE fp16 rounding away from the un-rounded chain at every link
    assert torch.equal(hi[0], plain[0])                              # the first launch has no residual: same C, plus its remainder
    assert rel(plain[3], ref) > 1.2 * rel(hi[3], ref) or rel(plain[3], ref) < 3e-4
    again = K.gemm(As[1], W, M, N, K_, bias=bias, residual=plain[0], **kw)
    assert torch.equal(again, plain[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# Every attention instantiation, both backward widths, the causal entry point and the option table against fp64 references.
# Each case prints the figures it asserts on (pytest -s / -rP shows them): the record of what a run measured.

# library defaults of the knobs the cases below move (g_opts in clora_gemm.hip); a value forwarded from the environment (capi._ENV_OPTIONS)
# is what a case restores
_OPTION_DEFAULTS = {"attn_fwd_waves": ("CLORA_ATTN_FWD_WAVES", 0), "attn_bwd_waves": ("CLORA_ATTN_BWD_WAVES", 0), "gn_blocks": ("CLORA_GN_BLOCKS", 512),
                    "epi_two_phase": ("CLORA_EPI_TWO_PHASE", 1), "gn_unroll": ("CLORA_GN_UNROLL", 0), "epi_hoist": ("CLORA_EPI_HOIST", 1),
                    "gn_resident": ("CLORA_GN_RESIDENT", 1), "wgrad_patch": ("CLORA_WGRAD_PATCH", 1), "strip_blocks": ("CLORA_STRIP_BLOCKS", 512),
                    "gn_team": ("CLORA_GN_TEAM", 2)}


def option_default(name):
    var, val = _OPTION_DEFAULTS[name]
    return int(os.environ.get(var) or val)


class options:
    """with options(attn_bwd_waves=8, ...): the knobs are set for the block and put back afterwards, whatever happens inside"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        for k_, v_ in self.kv.items():
            K.set_option(k_, v_)

    def __exit__(self, *exc):
        for k_ in self.kv:
            K.set_option(k_, option_default(k_))
        return False


def rel64(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def _attn_ref64(q, k, v, dO, B, H, Nq, Nk, D, scale, causal=False):
    """softmax(scale q k^T) v in fp64 on the fp16 inputs, one batch element at a time (the score tensor of a 4096-token site is 1 GiB per
    element): o [B*Nq, H*D], lse [B, H, Nq], the three gradients for dO, and the per-row size of the logits' terms
    scale * max_j sum_d |q_d k_jd| that the LSE bound of case_attention_full is built on."""
    o, lse, mag, dq, dk, dv = [], [], [], [], [], []
    heads = lambda t_, n: t_.double().reshape(n, H, D).permute(1, 0, 2)
    rows = lambda t_, n: t_.permute(1, 0, 2).reshape(n, H * D)
    for b in range(B):
        qb = heads(q[b * Nq:(b + 1) * Nq], Nq).clone().requires_grad_(dO is not None)
        kb = heads(k[b * Nk:(b + 1) * Nk], Nk).clone().requires_grad_(dO is not None)
        vb = heads(v[b * Nk:(b + 1) * Nk], Nk).clone().requires_grad_(dO is not None)
        s = qb @ kb.transpose(-1, -2) * scale
        if causal:
            s = s.masked_fill(torch.ones(Nq, Nk, dtype=torch.bool, device=s.device).triu(1), float("-inf"))
        ob = torch.softmax(s, -1) @ vb
        lse.append(torch.logsumexp(s.detach(), -1))
        mag.append((qb.detach().abs() @ kb.detach().abs().transpose(-1, -2)).amax(-1) * scale)
        o.append(rows(ob.detach(), Nq))
        if dO is not None:
            ob.backward(heads(dO[b * Nq:(b + 1) * Nq], Nq))
            dq.append(rows(qb.grad, Nq)), dk.append(rows(kb.grad, Nk)), dv.append(rows(vb.grad, Nk))
        del s, ob
    out = dict(o=torch.cat(o), lse=torch.stack(lse), mag=torch.stack(mag))
    if dO is not None:
        out.update(dq=torch.cat(dq), dk=torch.cat(dk), dv=torch.cat(dv))
    return out


def attention_full_inputs(dev, B, H, Nq, Nk, D, q_scale=1.0, seed=51):
    g = torch.Generator().manual_seed(seed)
    scale = D ** -0.5
    q = rnd((B * Nq, H * D), dev, g, q_scale)
    k, v, dO = rnd((B * Nk, H * D), dev, g), rnd((B * Nk, H * D), dev, g), rnd((B * Nq, H * D), dev, g)
    return dict(q=q, k=k, v=v, dO=dO, scale=scale, dims=(B, H, Nq, Nk, D), q_scale=q_scale, ref=_attn_ref64(q, k, v, dO, B, H, Nq, Nk, D, scale))


def attention_full_check(inp, strided=False, tag="", bwd=None):
    """one forward + backward of the library on prepared inputs, every output against the fp64 reference (case_attention_full);
    `bwd`: called in place of K.attn_bwd with its arguments (case_attention_workspace hands the C entry point a workspace of its own)"""
    bwd = bwd or K.attn_bwd
    B, H, Nq, Nk, D = inp["dims"]
    q, k, v, dO, scale, ref = inp["q"], inp["k"], inp["v"], inp["dO"], inp["scale"], inp["ref"]
    dev, HD = q.device, H * D
    o, lse = K.attn_fwd(q, k, v, B, H, Nq, Nk, D, scale)
    nan = float("nan")
    if strided:     # the gradients are column blocks of one buffer (a fused q | k | v projection's dgrad input) with 8 spare columns
        buf = torch.full((B * max(Nq, Nk), 3 * HD + 8), nan, dtype=f16, device=dev)
        dq, dk, dv = buf[:B * Nq, :HD], buf[:B * Nk, HD:2 * HD], buf[:B * Nk, 2 * HD:3 * HD]
    else:
        dq, dk, dv = (torch.full((n, HD), nan, dtype=f16, device=dev) for n in (B * Nq, B * Nk, B * Nk))
    bwd(q, k, v, o, dO, lse, B, H, Nq, Nk, D, scale, dq, dk, dv)
    errs = {"o": rel64(o, ref["o"])}
    # LSE, per row: the kernel rounds q * scale * log2(e) to fp16 once (<= 2^-12 relative per term of the logit); the factor 2 covers
    # the fp32 accumulation and log2f
    bound = 2.0 ** -11 * ref["mag"] + 1e-5
    lse_err = (lse.double() - ref["lse"]).abs()
    errs["lse"], errs["lse_bound"] = float(lse_err.max()), float(bound.max())
    errs["lse_margin"] = float((lse_err / bound).max())
    exact_zero = Nk == 1          # one key: every weight is exactly 1, dq and dk are exactly zero -- no relative error exists
    for name, got in (("dq", dq), ("dk", dk), ("dv", dv)):
        errs[name] = float(got.double().abs().max()) if (exact_zero and name != "dv") else rel64(got, ref[name])
    print(f"ATTN_FULL{tag} {inp['dims']} q_scale={inp['q_scale']} strided={strided} " + " ".join(f"{k_}={v_:.2e}" for k_, v_ in errs.items()))
    assert errs["o"] < 2e-3, ("o", errs)
    no_outliers(o, ref["o"], "o")
    assert bool((lse_err <= bound).all()), ("lse", errs)
    for name, got in (("dq", dq), ("dk", dk), ("dv", dv)):
        assert bool(torch.isfinite(got.float()).all()), (name, "not every element was written")
        assert errs[name] < (1e-4 if (exact_zero and name != "dv") else 4e-3), (name, errs)
        no_outliers(got, ref[name], name)
    if strided:
        spare = torch.ones(buf.shape, dtype=torch.bool, device=dev)
        spare[:B * Nq, :HD] = False
        spare[:B * Nk, HD:3 * HD] = False
        assert bool(torch.isnan(buf[spare].float()).all()), "the backward wrote outside its three column blocks"
    return (o, lse, dq.contiguous(), dk.contiguous(), dv.contiguous()), errs


def case_attention_full(dev, B, H, Nq, Nk, D, q_scale=1.0, strided=False):
    """clora_attn_fwd_f16 + clora_attn_bwd_f16 against fp64 on the same fp16 inputs: o (2e-3) and dq / dk / dv (4e-3) norm-wise and
    elementwise (no_outliers), the LSE under a per-row bound derived from the one fp16 rounding of the scaled query, every gradient
    element written (the buffers start as NaN), and with `strided` the gradients as column blocks of one wider buffer whose spare
    columns must stay untouched.  q_scale > 1: peaked softmax."""
    return attention_full_check(attention_full_inputs(dev, B, H, Nq, Nk, D, q_scale), strided)


ATTN_WIDTHS = [(bw, fw) for bw in (4, 8) for fw in (4, 6, 8, 16)]          # ("attn_bwd_waves", "attn_fwd_waves"); the first is the base


def case_attention_widths(dev, B, H, Nq, Nk, D, widths=ATTN_WIDTHS, strided=False):
    """case_attention_full under every block width of the forward (128 / 192 / 256 / 512 queries) and the backward (128 / 256 queries or
    keys): each passes the reference checks, and o, lse, dq, dk, dv are bit-identical to the 4-wave results (a block width only changes
    which workgroup owns which rows)."""
    inp = attention_full_inputs(dev, B, H, Nq, Nk, D)
    base = None
    for bw, fw in widths:
        with options(attn_bwd_waves=bw, attn_fwd_waves=fw):
            outs, _ = attention_full_check(inp, strided, tag=f"[bwd {bw} fwd {fw}]")
        if base is None:
            base = outs
        for name, a, b_ in zip(("o", "lse", "dq", "dk", "dv"), base, outs):
            assert torch.equal(a, b_), f"{name}: bwd {bw} / fwd {fw} waves differ from {widths[0]} in {int((a != b_).sum())} elements"


ATTN_OPERANDS = ("q", "k", "v", "o", "dO", "dq", "dk", "dv")      # the eight row-strided operands of the attention entry points


def attn_strides(HD):
    """eight pairwise different row strides, all multiples of 8 and at least HD + 16: every operand's column block starts at column 8
    of its own buffer and has spare columns on both sides"""
    return {name: HD + 8 * (i + 2) for i, name in enumerate(ATTN_OPERANDS)}


def _attn_arena(rows, HD, ld, max_ld, dev, gen=None):
    """a NaN-filled buffer of (rows + 2) * max_ld halves and the [rows, HD] column block at column 8 with row stride ld in it (random
    values with `gen`): an access with ANY of the eight strides stays inside the allocation, a read with another operand's stride picks
    up NaN, a store with another operand's stride lands on a NaN outside the block"""
    buf = torch.full(((rows + 2) * max_ld,), float("nan"), dtype=f16, device=dev)
    view = buf.as_strided((rows, HD), (ld, 1), 8)
    if gen is not None:
        view.copy_(rnd((rows, HD), dev, gen))
    return buf, view


def attention_strides_inputs(dev, B, H, Nq, Nk, D, causal=False, backward=True, seed=101):
    HD, scale = H * D, D ** -0.5
    ld = attn_strides(HD)
    g = torch.Generator().manual_seed(seed)
    rows = {name: B * (Nq if name in ("q", "o", "dO", "dq") else Nk) for name in ATTN_OPERANDS}
    inp = dict(dims=(B, H, Nq, Nk, D), scale=scale, ld=ld, rows=rows, causal=causal, backward=backward)
    for name in ("q", "k", "v") + (("dO",) if backward else ()):
        inp[name] = _attn_arena(rows[name], HD, ld[name], max(ld.values()), dev, g)[1]
    inp["ref"] = _attn_ref64(inp["q"], inp["k"], inp["v"], inp.get("dO"), B, H, Nq, Nk, D, scale, causal=causal)
    return inp


def attention_strides_check(inp, tag=""):
    """one forward (+ backward) on the inputs of attention_strides_inputs with fresh NaN-filled output buffers; every assertion names
    the output that is wrong"""
    B, H, Nq, Nk, D = inp["dims"]
    q, k, v, scale, ref, ld, rows = inp["q"], inp["k"], inp["v"], inp["scale"], inp["ref"], inp["ld"], inp["rows"]
    dev, HD, max_ld = q.device, H * D, max(inp["ld"].values())
    new = lambda name: _attn_arena(rows[name], HD, ld[name], max_ld, dev)

    def check(name, got, buf, lim):
        finite = bool(torch.isfinite(got.float()).all())
        e = rel64(got, ref[name]) if finite else float("nan")
        print(f"ATTN_STRIDES{tag} {inp['dims']} causal={inp['causal']} {name}={e:.2e}")
        assert finite, (name, "not every element is finite: unwritten, or computed from an operand read with another operand's row stride")
        assert e < lim, (name, e)
        try:
            no_outliers(got, ref[name], name)
        except AssertionError as err:
            raise AssertionError((name, str(err))) from None
        rest = buf.clone()
        rest.as_strided((rows[name], HD), (ld[name], 1), 8).fill_(float("nan"))
        assert bool(torch.isnan(rest.float()).all()), (name, "the kernel wrote outside the operand's column block")

    obuf, o = new("o")
    if inp["causal"]:
        assert Nq == Nk
        K.attn_fwd_causal(q, k, v, B, H, Nq, D, scale, out=o)
        lse = None
    else:
        _, lse = K.attn_fwd(q, k, v, B, H, Nq, Nk, D, scale, out=o)
    check("o", o, obuf, 2e-3)
    if lse is not None:
        bound = 2.0 ** -11 * ref["mag"] + 1e-5               # attention_full_check: the one fp16 rounding of the scaled query
        lse_err = (lse.double() - ref["lse"]).abs()
        assert bool(torch.isfinite(lse).all()) and bool((lse_err <= bound).all()), ("lse", float(lse_err.max()), float(bound.max()))
    if not inp["backward"]:
        return
    (qbuf, dq), (kbuf, dk), (vbuf, dv) = new("dq"), new("dk"), new("dv")
    K.attn_bwd(q, k, v, o, inp["dO"], lse, B, H, Nq, Nk, D, scale, dq, dk, dv)
    for name, got, buf in (("dq", dq, qbuf), ("dk", dk, kbuf), ("dv", dv, vbuf)):
        check(name, got, buf, 4e-3)


def case_attention_strides(dev, B, H, Nq, Nk, D, causal=False, waves=(0,)):
    """The eight leading dimensions of the attention entry points are independent: q, k, v, o, dO, dq, dk, dv are each a column block
    (from column 8) of a NaN-filled buffer of its own, under eight pairwise different row strides.  Against fp64 on the same inputs: o
    within 2e-3, dq / dk / dv within 4e-3 norm-wise and without outliers, the LSE under the bound of case_attention_full, every output
    element finite, and everything outside an output's block still NaN.  A kernel that addresses one operand with another's stride reads
    NaN or stores outside its block; the buffers are sized so that even then no access leaves them.  causal: clora_attn_fwd_causal_f16
    with its four strides, forward only.  waves: the "attn_bwd_waves" / "attn_fwd_waves" values to run under (0 = the library's choice)."""
    inp = attention_strides_inputs(dev, B, H, Nq, Nk, D, causal=causal, backward=not causal)
    for w in waves:
        if not w:
            attention_strides_check(inp)
            continue
        with options(attn_bwd_waves=w, attn_fwd_waves=w):
            attention_strides_check(inp, tag=f"[{w} waves]")


def attn_bwd_workspace_bytes(dev, B, H, Nk, D):
    """what K.attn_bwd hands clora_attn_bwd_f16 as its split workspace"""
    return K.workspace(16 * 2 * B * Nk * H * D * 4, dev).numel() if Nk <= 1024 else 0


def attn_split_count(B, H, Nq, Nk, D, workspace_bytes):
    """The number of query splits of clora_attn_bwd_f16's dK/dV launch, restated from its host code: fewer than 256 blocks of 128 keys
    and at least 512 queries split into ns = min(512 / key blocks, Nq / 128, workspace / one fp32 dK | dV slab pair) parts of
    q_per_split = cdiv(Nq, ns) rounded up to 64 rows.  1: the unsplit kernel."""
    cdiv = lambda a, b_: -(-a // b_)
    kv_blocks = cdiv(Nk, 128) * B * H
    if kv_blocks >= 256 or Nq < 512 or workspace_bytes <= 0 or D % 4:
        return 1
    ns = min(512 // kv_blocks, Nq // 128, workspace_bytes // (2 * B * Nk * H * D * 4))
    return cdiv(Nq, cdiv(cdiv(Nq, ns), 64) * 64) if ns > 1 else 1


def case_attention_split(dev, B, H, Nq, Nk, D, splits, strided=True, tail=False):
    """case_attention_full on a shape that takes the query-split dK/dV path (per-split fp32 slabs, folded by attn_dkv_convert_kernel).
    The split count the shape is chosen for is asserted from the restated rule, so a change of the rule fails here instead of silently
    leaving the path.  tail: the fold's unrolled group of four slab pairs is followed by a tail of two or three."""
    got = attn_split_count(B, H, Nq, Nk, D, attn_bwd_workspace_bytes(dev, B, H, Nk, D))
    assert got == splits, f"{(B, H, Nq, Nk, D)} is split {got} ways, the case was written for {splits}"
    assert not tail or (got >= 6 and got % 4 >= 2), f"{got} splits: no fold tail of two or more slab pairs after a full group"
    return case_attention_full(dev, B, H, Nq, Nk, D, strided=strided)


WS_SENTINEL = 0xA5


def case_attention_workspace(dev, B, H, Nq, Nk, D, pairs=2.5):
    """clora_attn_bwd_f16 called directly with a workspace_bytes of `pairs` slab pairs on a shape that would take more splits: the same
    fp64 checks as case_attention_full, and every byte past the stated budget keeps its sentinel (the region is the head of a larger
    buffer that holds the Nq / 128 slab pairs no split count can exceed, so an ignored budget is seen, not a stray store).  Then the
    same shape with a NULL workspace: the unsplit kernel on a shape that would otherwise split."""
    from controllora_amd import capi
    slab = 2 * B * Nk * H * D * 4
    budget = int(pairs * slab)
    free, held = attn_split_count(B, H, Nq, Nk, D, 1 << 62), attn_split_count(B, H, Nq, Nk, D, budget)
    assert 1 < held < free, f"{(B, H, Nq, Nk, D)}: {free} splits without a budget, {held} under {pairs} slab pairs"
    inp = attention_full_inputs(dev, B, H, Nq, Nk, D)
    arena = torch.full(((Nq // 128) * slab + 64,), WS_SENTINEL, dtype=torch.uint8, device=dev)

    def bwd_with(ws, nbytes):
        def bwd(q, k, v, o, dO, lse, B, H, Nq, Nk, D, scale, dq, dk, dv):
            delta = torch.empty((B, H, Nq), dtype=f32, device=q.device)
            capi.lib().call("clora_attn_bwd_f16", capi.ptr(q, f16), q.stride(0), capi.ptr(k, f16), k.stride(0), capi.ptr(v, f16), v.stride(0),
                            capi.ptr(o, f16), o.stride(0), capi.ptr(dO, f16), dO.stride(0), capi.ptr(lse, f32), capi.ptr(delta),
                            capi.ptr(dq, f16), dq.stride(0), capi.ptr(dk, f16), dk.stride(0), capi.ptr(dv, f16), dv.stride(0),
                            B, H, Nq, Nk, D, float(scale), capi.ptr(ws), nbytes, capi.stream())
        return bwd

    attention_full_check(inp, strided=True, tag=f"[{pairs} slab pairs]", bwd=bwd_with(arena, budget))
    past = int((arena[budget:] != WS_SENTINEL).sum())
    assert past == 0, ("workspace", f"{past} bytes past the stated {budget} were written")
    assert bool((arena[:held * slab] != WS_SENTINEL).any()), ("workspace", "the split path did not run")
    attention_full_check(inp, strided=True, tag="[no workspace]", bwd=bwd_with(None, 0))
    assert bool((arena[budget:] == WS_SENTINEL).all()), ("workspace", "written by a call that was given none")


def case_attention_causal(dev, B, H, N, D, strided=True):
    """clora_attn_fwd_causal_f16 against an fp64 masked softmax (2e-3: the limit of the unmasked forward, same kernel template) and
    elementwise; row 0 sees one key with weight exactly 1, so it equals v[0] bit for bit; keys and values at positions >= N // 2 are
    invisible to the rows before them (those rows keep their bits when they change) and visible to the rest.  strided: q | k | v are column blocks of one buffer (the
    self-attention layout) and the output a column block of a wider NaN-filled one."""
    g = torch.Generator().manual_seed(57)
    HD, scale = H * D, D ** -0.5
    if strided:
        qkv = rnd((B * N, 3 * HD), dev, g)
        q, k, v = qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:]
        obuf = torch.full((B * N, HD + 16), float("nan"), dtype=f16, device=dev)
        out = obuf[:, 8:8 + HD]
    else:
        q, k, v = (rnd((B * N, HD), dev, g) for _ in range(3))
        obuf, out = None, torch.full((B * N, HD), float("nan"), dtype=f16, device=dev)
    o = K.attn_fwd_causal(q, k, v, B, H, N, D, scale, out=out)
    ref = _attn_ref64(q, k, v, None, B, H, N, N, D, scale, causal=True)["o"]
    e, worst = rel64(o, ref), float((o.double() - ref).abs().max())
    print(f"ATTN_CAUSAL {(B, H, N, D)} strided={strided} o={e:.2e} worst={worst:.2e}")
    assert bool(torch.isfinite(o.float()).all()), "not every output element was written"
    assert e < 2e-3, e
    no_outliers(o, ref, "causal o")
    if strided:
        assert bool(torch.isnan(obuf[:, :8].float()).all()) and bool(torch.isnan(obuf[:, 8 + HD:].float()).all())
    o3, v3 = o.reshape(B, N, HD), v.reshape(B, N, HD)
    assert torch.equal(o3[:, 0], v3[:, 0]), "row 0 attends to key 0 alone"
    half = N // 2
    k2, v2 = k.clone().reshape(B, N, HD), v.clone().reshape(B, N, HD)
    k2[:, half:], v2[:, half:] = rnd((B, N - half, HD), dev, g), rnd((B, N - half, HD), dev, g)
    o2 = K.attn_fwd_causal(q, k2.reshape(B * N, HD), v2.reshape(B * N, HD), B, H, N, D, scale).reshape(B, N, HD)
    assert torch.equal(o2[:, :half], o3[:, :half]), "a row changed with keys it must not see"
    assert bool((o2[:, half:] != o3[:, half:]).any(-1).all()), "a row did not change with keys it sees"


def case_attention_causal_rejects(dev, D=72):
    """head dims above 64 are outside clora_attn_fwd_causal_f16's contract: CLORA_ERR_ARG, nothing launched (the output keeps its bits)"""
    from controllora_amd import capi
    g = torch.Generator().manual_seed(58)
    q, k, v = (rnd((16, D), dev, g) for _ in range(3))
    out = torch.full((16, D), float("nan"), dtype=f16, device=dev)
    try:
        K.attn_fwd_causal(q, k, v, 1, 1, 16, D, D ** -0.5, out=out)
    except capi.CloraError as e:
        assert "bad argument" in str(e), e
    else:
        raise AssertionError(f"D = {D} was accepted")
    assert bool(torch.isnan(out.float()).all())


def case_groupnorm_offset(dev, B, HW, C, G, offset, silu=False, check=True, eps=1e-5, seed=61):
    """GroupNorm of unit-variance inputs centred at `offset` (|mean| / std = offset; every other GroupNorm case has 0.2): output and
    statistics (8e-4) and dx (2e-3) against fp64 under every plan the shape can take ("gn_resident" 0 / 1 x "gn_team" 0 / 2).  The
    statistics are one pass of fp32 sums over x - P (P: one sample of the group, gn_pivot in clora_norm.hip); plain E[x^2] - mean^2 lost
    about offset^2 * 2^-24 of the variance and failed this case at offset 100 on the two-launch plan.  check=False: print only."""
    g = torch.Generator().manual_seed(seed)
    x = (rnd((B, HW, C), dev, g, dtype=f32) + offset).half()
    gamma, beta = (1 + 0.2 * rnd((C,), dev, g, dtype=f32)), 0.2 * rnd((C,), dev, g, dtype=f32)
    dy = rnd((B, HW, C), dev, g)
    x64 = x.double().clone().requires_grad_(True)
    y = F.group_norm(x64.permute(0, 2, 1), G, gamma.double(), beta.double(), eps).permute(0, 2, 1)
    if silu:
        y = F.silu(y)
    y.backward(dy.double())
    xg = x.double().reshape(B, HW, G, C // G)
    mean = xg.mean((1, 3))
    rstd = (xg.var((1, 3), unbiased=False) + eps).rsqrt()
    worst = {}
    for resident in (0, 1):
        for team in (0, 2):
            with options(gn_resident=resident, gn_team=team):
                out, stats = K.groupnorm_fwd(x, gamma, beta, G, eps, silu)
                dx, _, _ = K.groupnorm_bwd(x, dy, gamma, beta, stats, G, silu)
            errs = dict(y=rel64(out, y), mean=rel64(stats[..., 0], mean), rstd=rel64(stats[..., 1], rstd), dx=rel64(dx, x64.grad))
            print(f"GN_OFFSET {(B, HW, C, G)} offset={offset} silu={silu} gn_resident={resident} gn_team={team} " +
                  " ".join(f"{k_}={v_:.2e}" for k_, v_ in errs.items()))
            assert all(math.isfinite(v_) for v_ in errs.values()), errs
            if check:
                assert errs["y"] < 8e-4 and errs["mean"] < 8e-4 and errs["rstd"] < 8e-4 and errs["dx"] < 2e-3, (resident, team, errs)
                no_outliers(out, y, "groupnorm y")
            for k_, v_ in errs.items():
                worst[k_] = max(worst.get(k_, 0.0), v_)
    assert K.gn_team_errors(x.device) == 0
    return worst



# ---- the team GroupNorm kernels at narrow slabs and large teams (the VAE's norms), and which plan a call took
def team_generations(dev):
    """the 32 generation words of the team GroupNorm exchange state (byte 256 of K.gn_team_state, layout beside kTeamHeader in
    clora_norm.hip and in INTEGRATION.md) as a list of ints.  A team launch of U = B * slabs units advances exactly the first U words,
    every other plan advances none: the difference around a call says which plan it took, members = 256 / U."""
    words = K.gn_team_state(dev)[256:256 + 4 * 32].cpu().view(torch.int32)
    return [int(w) & 0xFFFFFFFF for w in words]


_TEAM_STEP = {}


def team_step(dev):
    """what ONE team launch adds to the generation words of its units: measured once per library on a shape the suite has always run
    on the team plan, (1, 1024, 320, 32) = 2 slabs of 160 channels (the emulator issues a launch as two passes over the blocks, see
    gn_team_launch: whatever that makes of the count is read here, not assumed).  The real library: exactly 1."""
    from controllora_amd import capi
    key = (str(dev), capi.lib().path)
    if key not in _TEAM_STEP:
        g = torch.Generator().manual_seed(90)
        x = rnd((1, 1024, 320), dev, g)
        gamma, beta = 1 + 0.2 * rnd((320,), dev, g, dtype=f32), 0.2 * rnd((320,), dev, g, dtype=f32)
        with options(gn_team=2):
            before = team_generations(dev)
            K.groupnorm_fwd(x, gamma, beta, 32, 1e-5, True)
            after = team_generations(dev)
        d = [(a - b) & 0xFFFFFFFF for a, b in zip(after, before)]
        assert d[0] >= 1 and d[:2] == [d[0]] * 2 and d[2:] == [0] * 30, f"(1, 1024, 320, 32) forward is not a 2-unit team launch: {d}"
        if str(dev) != "cpu":
            assert d[0] == 1, d
        _TEAM_STEP[key] = d[0]
    return _TEAM_STEP[key]


class expect_team:
    """with expect_team(dev, units, launches=1): the block's GroupNorm calls were `launches` team launches of `units` units each
    (units = 0: none of them took a team kernel), told by the generation words alone"""

    def __init__(self, dev, units, launches=1, what=""):
        self.dev, self.units, self.launches, self.what = dev, units, launches, what

    def __enter__(self):
        self.step = team_step(self.dev)
        self.before = team_generations(self.dev)
        return self

    def __exit__(self, *exc):
        if exc[0] is None:
            after = team_generations(self.dev)
            d = [(a - b) & 0xFFFFFFFF for a, b in zip(after, self.before)]
            want = [self.step * self.launches] * self.units + [0] * (32 - self.units)
            assert d == want, f"{self.what}: expected {self.launches} team launch(es) of {self.units} units ({256 // max(self.units, 1)} members), " \
                              f"the generation words moved by {d}"
        return False


# (B, HW, C, G, units forward, units backward) at "gn_team" 2, by hand from gn_team_plan (clora_norm.hip); members = 256 / units
TEAM_NARROW_SHAPES = [
    (4, 4096, 16, 8, 4, 4),      # the VAE encoder's first norm at resolution 64: CS = 16 (two chunks per row), 64 members, 64 of 256 row lanes own a row
    (2, 4096, 16, 8, 2, 2),      # ... at the short batch: 128 members over the same generation words and granule slots
    (4, 1024, 16, 8, 4, 4),      # its 32x32 norms
    (4, 1024, 32, 8, 4, 4),
    (1, 4096, 16, 8, 1, 1),      # one unit: 256 members = the sweep's cap at GK = 16 (8 x 512 / 16), 8 granules per thread
    (2, 1030, 64, 8, 2, 2),      # ragged: 128 members of 9 rows, members 115 .. 127 begin past the last row
    (4, 4096, 128, 32, 4, 4),    # CS just under 160 with 4-channel groups: GK = 64, the first feasible split is taken
    (4, 4096, 512, 32, 8, 8),    # the SD-1.5 VAE mid block: two slabs of 256
    (2, 4096, 512, 32, 4, 4),    # ... one slab would need 128 members at GK = 64 (cap 64): two slabs of 256, 64 members
]

# ("gn_team", B, HW, C, G, units forward, units backward, run the backward): the 16x16 and 8x8 maps under the levels that admit them
# (3: HW >= 256 both ways; 4: HW >= 64) and under the default.  A shape whose one-block-per-slab plan holds at most "defer_max_rows"
# (4) rows per thread keeps that plan at EVERY level (gn_fwd_impl / gn_bwd_impl: fold_shape, so that deferring a producer never changes
# the bits): (4, 256, 32, 8) and (4, 64, 64, 8) are such shapes and must stay off the team kernels; (4, 256, 64, 8) (8 rows per thread)
# and (2, 64, 640, 4) (160-channel groups, 6 rows per thread) are the smallest that leave it.
TEAM_LEVEL_SHAPES = [(3, 4, 256, 32, 8, 0, 0, True), (4, 4, 64, 64, 8, 0, 0, True),
                     (3, 4, 256, 64, 8, 4, 4, True), (2, 4, 256, 64, 8, 0, 4, True),
                     (4, 2, 64, 640, 4, 8, 8, True), (3, 2, 64, 640, 4, 0, 0, True), (2, 2, 64, 640, 4, 0, 0, True)]


def case_groupnorm_team_narrow(dev, B, HW, C, G, silu, level=2, units=None, units_bwd=None, offset=None, backward=True, eps=1e-5, seed=91):
    """The team kernels where the UNet shapes never take them: slabs narrower than 160 channels (the planner's first-feasible branch, a
    thread map in which most row lanes own no row, gn_res_reduce with 8 threads per channel), teams of 128 and 256 members (4 - 8
    granules per sweeping thread), ragged last members, and the maps that only "gn_team" 3 / 4 put on them.
      - the plan is asserted, not assumed: `units` (forward) / `units_bwd` team units per launch by the generation words, 0 = no team;
      - y, statistics (8e-4) and dx with and without dres (2e-3) against fp64 torch on the same fp16 inputs (case_groupnorm's limits);
      - against "gn_team" 0 on the same inputs: 2e-4 / 1e-5 / 3e-4 (include/clora.h, the table above clora_set_option);
      - three more identical calls give the bits of the first, and no exchange gave up.
    Inputs as in case_groupnorm (x * 1.5 + 0.3), or unit variance around `offset` (case_groupnorm_offset: the pivot is shared by all
    members of a unit)."""
    units_bwd = units if units_bwd is None else units_bwd
    team_step(dev)                                               # measured before the level is set: it moves "gn_team" itself
    g = torch.Generator().manual_seed(seed)
    if offset is None:
        x = (rnd((B, HW, C), dev, g).float() * 1.5 + 0.3).half()
    else:
        x = (rnd((B, HW, C), dev, g, dtype=f32) + offset).half()
    gamma, beta = (1 + 0.2 * rnd((C,), dev, g, dtype=f32)), 0.2 * rnd((C,), dev, g, dtype=f32)
    dy, dres = rnd((B, HW, C), dev, g), rnd((B, HW, C), dev, g)
    x64 = x.double().clone().requires_grad_(True)
    y = F.group_norm(x64.permute(0, 2, 1), G, gamma.double(), beta.double(), eps).permute(0, 2, 1)
    if silu:
        y = F.silu(y)
    y.backward(dy.double())
    xg = x.double().reshape(B, HW, G, C // G)
    mean, rstd = xg.mean((1, 3)), (xg.var((1, 3), unbiased=False) + eps).rsqrt()
    tag = f"GN_TEAM_NARROW {(B, HW, C, G)} level={level} offset={offset} silu={silu}"

    def run():
        with expect_team(dev, units, what=tag + " forward"):
            out, stats = K.groupnorm_fwd(x, gamma, beta, G, eps, silu)
        if not backward:
            return out, stats, None, None
        with expect_team(dev, units_bwd, 2, what=tag + " backward"):
            dx, _, _ = K.groupnorm_bwd(x, dy, gamma, beta, stats, G, silu)
            dx2, _, _ = K.groupnorm_bwd(x, dy, gamma, beta, stats, G, silu, dres=dres)
        return out, stats, dx, dx2

    with options(gn_team=level):
        out, stats, dx, dx2 = run()
        again = [run() for _ in range(3)]
    with options(gn_team=0), expect_team(dev, 0, what=tag + " gn_team=0"):
        out0, stats0 = K.groupnorm_fwd(x, gamma, beta, G, eps, silu)
        dx0 = K.groupnorm_bwd(x, dy, gamma, beta, stats0, G, silu, dres=dres)[0] if backward else None
    errs = dict(y=rel64(out, y), mean=rel64(stats[..., 0], mean), rstd=rel64(stats[..., 1], rstd))
    across = dict(y=rel64(out, out0), stats=rel64(stats, stats0))
    if backward:
        errs.update(dx=rel64(dx, x64.grad), dx_res=rel64(dx2, x64.grad + dres.double()))
        across.update(dx=rel64(dx2, dx0))
    print(tag, "units", (units, units_bwd), " ".join(f"{k_}={v_:.2e}" for k_, v_ in errs.items()),
          "| vs gn_team=0", " ".join(f"{k_}={v_:.2e}" for k_, v_ in across.items()))
    assert errs["y"] < 8e-4 and errs["mean"] < 8e-4 and errs["rstd"] < 8e-4, errs
    no_outliers(out, y, tag + " y")
    assert across["y"] < 2e-4 and across["stats"] < 1e-5, across
    if backward:
        assert errs["dx"] < 2e-3 and errs["dx_res"] < 2e-3, errs
        no_outliers(dx, x64.grad, tag + " dx")
        assert across["dx"] < 3e-4, across
    for i, rerun in enumerate(again):
        for name, a, b_ in zip(("y", "stats", "dx", "dx + dres"), rerun, (out, stats, dx, dx2)):
            assert a is None or torch.equal(a, b_), f"{tag}: {name} of identical call {i + 2} differs from the first " \
                                                    f"({int((a != b_).sum())} elements, rel {rel64(a, b_):.2e})"
    assert K.gn_team_errors(dev) == 0
    return errs


def case_groupnorm_team_alternating(dev, graph=False):
    """The launch sequence of a training run whose epochs end in a short batch (the VAE encoder's team norms at resolution 64, batch
    4, 2, 4, 2): 4 units of 64 members and 2 units of 128 members alternate over the same generation words and granule slots, a GEMM
    between the launches so that workgroups start unevenly.  Four repetitions of forward + backward at (4, 4096, 16), (4, 1024, 32),
    (2, 4096, 16), (2, 1024, 32), G = 8:
      - every repetition gives the bits of the first, and the generation words moved as the plan says (units 0, 1 by every launch,
        units 2, 3 by the batch-4 launches only);
      - the same sequence on a freshly zeroed state gives the same bits (the old state is put back, never freed: graphs hold it);
      - graph (the real library only): the batch-4 pair captured in one graph and replayed five times with eager batch-2 launches
        between the replays; every replay and every eager launch gives the bits of the first eager pass.
    A determinism check of 4 + 4 + 5 rounds, not a loop that hunts for a failure."""
    g = torch.Generator().manual_seed(92)
    G = 8
    data = []
    for B, HW, C in ((4, 4096, 16), (4, 1024, 32), (2, 4096, 16), (2, 1024, 32)):
        x, dy = (rnd((B, HW, C), dev, g).float() * 1.5 + 0.3).half(), rnd((B, HW, C), dev, g)
        gamma, beta = 1 + 0.2 * rnd((C,), dev, g, dtype=f32), 0.2 * rnd((C,), dev, g, dtype=f32)
        data.append((x, dy, gamma, beta))
    A, W = rnd((1024, 64), dev, g), rnd((64, 64), dev, g)

    def launches(items):
        outs = []
        for x, dy, gamma, beta in items:
            y, st = K.groupnorm_fwd(x, gamma, beta, G, 1e-5, True)
            K.gemm(A, W, 1024, 64, 64)
            dx, _, _ = K.groupnorm_bwd(x, dy, gamma, beta, st, G, True)
            outs += [y, st, dx]
        return outs

    def sequence(what):
        step = team_step(dev)
        before = team_generations(dev)
        reps = [launches(data) for _ in range(4)]
        d = [(a - b) & 0xFFFFFFFF for a, b in zip(team_generations(dev), before)]
        assert d == [32 * step] * 2 + [16 * step] * 2 + [0] * 28, (what, d)
        for r, rep in enumerate(reps[1:]):
            for i, (a, b_) in enumerate(zip(rep, reps[0])):
                assert torch.equal(a, b_), f"{what}: repetition {r + 2}, output {i} (shape {tuple(a.shape)}) differs from the first repetition " \
                                           f"in {int((a != b_).sum())} elements"
        return reps[0]

    step = team_step(dev)
    with options(gn_team=2):
        first = sequence("persistent state")
        key = K._dev_key(dev)
        old = K._gn_team[key]
        K._gn_team[key] = torch.zeros_like(old)
        try:
            fresh = sequence("zeroed state")
            assert team_generations(dev) == [32 * step] * 2 + [16 * step] * 2 + [0] * 28
            assert K.gn_team_errors(dev) == 0
        finally:
            K._gn_team[key] = old
        for i, (a, b_) in enumerate(zip(fresh, first)):
            assert torch.equal(a, b_), f"zeroed state: output {i} differs from the persistent state's in {int((a != b_).sum())} elements"
        if graph:
            torch.cuda.synchronize()
            cg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(cg):
                captured = launches(data[:2])
            for rnd_ in range(5):
                cg.replay()
                eager = launches(data[2:])
                torch.cuda.synchronize()
                for i, (a, b_) in enumerate(zip(captured + eager, first)):
                    assert torch.equal(a, b_), f"round {rnd_}: output {i} ({'replay' if i < 6 else 'eager'}) differs from the first eager pass " \
                                               f"in {int((a != b_).sum())} elements"
    assert K.gn_team_errors(dev) == 0


def case_lora_down_mode(dev, mode, M, Kd):
    """option "lora_down_mode": three stacked rank-4 down-projections with a second input on the first, against fp32 torch (1e-5: fp32
    summation-order noise) and elementwise; two launches in one mode give the same bits"""
    g = torch.Generator().manual_seed(61)
    X, X2 = rnd((M, Kd), dev, g), rnd((M, Kd), dev, g)
    D = rnd((12, Kd), dev, g, 0.25, dtype=f32)
    ref = X.float() @ D.T
    ref[:, :4] += X2.float() @ D[:4].T
    try:
        K.set_option("lora_down_mode", mode)
        T = torch.empty((M, 12), dtype=f32, device=dev)
        K.lora_down_multi([K.down_job(X, D, T, 0, M, Kd, X2=X2, r2=4)])
        again = torch.empty_like(T)
        K.lora_down_multi([K.down_job(X, D, again, 0, M, Kd, X2=X2, r2=4)])
    finally:
        K.set_option("lora_down_mode", 1)                   # the library default
    assert rel(T, ref) < 1e-5 and torch.equal(T, again), (mode, M, Kd, rel(T, ref))
    no_outliers(T, ref, f"lora_down mode {mode} M={M} K={Kd}")


# ---- the option table (include/clora.h above clora_set_option): a launch set per knob, run at the default and at another value
def _launches_epilogue(dev, big):
    """the projection epilogues on the 8-wave tiles 51..58.  Each entry: (label, output, fp64-derived reference, rel limit, exact) --
    exact: the header promises the same bits at every setting of "epi_hoist" / "epi_two_phase" for this launch"""
    from controllora_amd import ops
    g = torch.Generator().manual_seed(91)
    M, N, K_ = (4100, 320, 320) if big else (300, 320, 128)
    A, B = rnd((M, K_), dev, g), rnd((N, K_), dev, g, 1 / math.sqrt(K_))
    bias, res, rowadd = rnd((N,), dev, g, dtype=f32), rnd((M, N), dev, g), rnd((4, N), dev, g)
    T, U, Ut = rnd((M, 8), dev, g, dtype=f32), rnd((N, 4), dev, g, dtype=f32), rnd((4, N), dev, g, dtype=f32)
    base = A.double() @ B.double().T
    seg = torch.arange(N, device=dev) // (N // 2)
    lora = torch.stack([T[:, :4].double() @ U[n].double() if int(s_) == 0 else T[:, 4:].double() @ U[n].double() for n, s_ in enumerate(seg.tolist())], 1)
    fin = lambda pre: pre.float().half().float() + res.float()           # the epilogue rounds once, then adds the residual
    out = []
    for tile in range(51, 59):
        kw = dict(tile_cfg=tile, split_k=1, _tuned=False)
        out.append((f"tile {tile} bias+adapter(2 segments)+residual",
                    K.gemm(A, B, M, N, K_, bias=bias, residual=res, lora_t=T, lora_u=U, lora_seg=N // 2, lora_scale=0.7, **kw),
                    fin(base + bias.double() + 0.7 * lora), 6e-4, False))
        T4 = T[:, :4].contiguous()
        out.append((f"tile {tile} adapter(lora_u_tr)+residual",
                    K.gemm(A, B, M, N, K_, residual=res, lora_t=T4, lora_u=Ut, lora_seg=N, lora_u_tr=True, lora_r=4, **kw),
                    fin(base + T4.double() @ Ut.double()), 6e-4, False))
        out.append((f"tile {tile} bias+residual", K.gemm(A, B, M, N, K_, bias=bias, residual=res, **kw), fin(base + bias.double()), 6e-4, True))
        kw["split_k"] = 2
        out.append((f"tile {tile} split-K 2 bias+rowadd+adapter+residual",
                    K.gemm(A, B, M, N, K_, bias=bias, rowadd=rowadd, rows_per_batch=M // 4, residual=res, lora_t=T, lora_u=U, lora_seg=N // 2,
                           lora_scale=0.7, **kw),
                    fin(base + bias.double() + rowadd.double().repeat_interleave(M // 4, 0) + 0.7 * lora), 6e-4, False))
    Dm = rnd((4, K_), dev, g, 1 / math.sqrt(K_), dtype=f32)                # the adapter's down-projection evaluated inside the launch
    pack = ops.ADAPTER_PACKS.get([Dm])
    T_ref = A.double() @ Dm.double().T
    for tile in (55, 0):
        Tw = torch.full((M, 4), float("nan"), dtype=f32, device=dev)
        y = K.gemm(A, B, M, N, K_, bias=bias, residual=res, lora_t=Tw, lora_u=U, lora_seg=N, lora_scale=0.7, lora_r=4, lora_dpack=pack,
                   tile_cfg=tile, split_k=1, _tuned=False)
        out.append((f"tile {tile} lora_dpack y", y, fin(base + bias.double() + 0.7 * (T_ref @ U.double().T)), 6e-4, True))
        out.append((f"tile {tile} lora_dpack T", Tw, T_ref, 2e-6, True))
    return out


def _launches_groupnorm(dev, big):
    """forward and backward under "gn_resident" 0 and 1.  exact (the same bits at every "gn_blocks"): the one-launch plans, which do
    not chunk rows -- `one_launch` shapes under gn_resident 1, team shapes always; the two-launch scheme re-partitions its fp32 sums"""
    shapes = [(2, 300, 320, 32, "one_launch"), (2, 64, 1280, 32, "one_launch"), (1, 1100, 64, 8, "any")]
    if big:
        shapes = [(4, 256, 1280, 32, "one_launch"), (4, 4096, 320, 32, "team"), (3, 1000, 640, 32, "any"), (2, 300, 320, 32, "one_launch")]
    out = []
    for B, HW, C, G, kind in shapes:
        g = torch.Generator().manual_seed(HW + C)
        x = (rnd((B, HW, C), dev, g).float() * 1.5 + 0.3).half()
        gamma, beta = (1 + 0.2 * rnd((C,), dev, g, dtype=f32)), 0.2 * rnd((C,), dev, g, dtype=f32)
        dy, dres = rnd((B, HW, C), dev, g), rnd((B, HW, C), dev, g)
        x64 = x.double().clone().requires_grad_(True)
        y = F.silu(F.group_norm(x64.permute(0, 2, 1), G, gamma.double(), beta.double(), 1e-5).permute(0, 2, 1))
        y.backward(dy.double())
        for resident in (0, 1):
            with options(gn_resident=resident):
                o, st = K.groupnorm_fwd(x, gamma, beta, G, 1e-5, True)
                dx, _, _ = K.groupnorm_bwd(x, dy, gamma, beta, st, G, True, dres=dres)
            exact = kind == "team" or (kind == "one_launch" and resident == 1)
            tag = f"{(B, HW, C, G)} gn_resident {resident}"
            out += [(f"{tag} y", o, y.detach(), 8e-4, exact, 2e-4), (f"{tag} stats", st, None, None, exact, 1e-5),
                    (f"{tag} dx", dx, x64.grad + dres.double(), 2e-3, exact, 3e-4)]
    return out


def _launches_strip(dev, big):
    """the strip convolution (tile_cfg 61), forward + bias and dgrad, on maps tall enough for the block count to change the row ranges"""
    import ctypes
    from controllora_amd import capi
    out = []
    for Bn, H, W, Ci, Co in ([(4, 512, 512, 32, 32), (2, 256, 256, 32, 64)] if big else [(1, 40, 128, 32, 32), (2, 24, 128, 32, 64)]):
        g = torch.Generator().manual_seed(H + Co)
        x, w = rnd((Bn, Ci, H, W), dev, g), rnd((Co, Ci, 3, 3), dev, g, 1 / math.sqrt(9 * Ci))
        bias, dy = rnd((Co,), dev, g, dtype=f32), rnd((Bn, Co, H, W), dev, g)
        xin = x.float().clone().requires_grad_(True)               # fp32 torch, as in case_conv_strip (K = 288 / 576 products)
        y = F.conv2d(xin, w.float(), bias.float(), padding=1)
        y.backward(dy.float())
        M = Bn * H * W
        xn = x.permute(0, 2, 3, 1).contiguous().reshape(M, Ci)
        wp = w.permute(0, 2, 3, 1).contiguous().reshape(Co, 9 * Ci)
        cd, _, _ = K.conv_fwd_desc(H, W, Ci, 3, 1, 1)
        assert capi.lib().cdll.clora_conv_strip_eligible(M, Co, ctypes.byref(cd)) == 1
        out.append((f"strip fwd {(Bn, H, W, Ci, Co)}", K.gemm(xn, wp, M, Co, 9 * Ci, conv=cd, bias=bias),
                    y.detach().permute(0, 2, 3, 1).reshape(M, Co), 6e-4, True))
        wd = w.permute(1, 2, 3, 0).contiguous().reshape(Ci, 9 * Co)
        dyn = dy.permute(0, 2, 3, 1).contiguous().reshape(M, Co)
        cdd = K.conv_dgrad_desc(H, W, Co, H, W, 3, 1, 1)
        if capi.lib().cdll.clora_conv_strip_eligible(M, Ci, ctypes.byref(cdd)) == 1:
            out.append((f"strip dgrad {(Bn, H, W, Ci, Co)}", K.gemm(dyn, wd, M, Ci, 9 * Co, conv=cdd),
                        xin.grad.permute(0, 2, 3, 1).reshape(M, Ci), 6e-4, True))
    assert len(out) >= 3, "no shape took the strip dgrad"
    return out


def _launches_wgrad_patch(dev, big):
    """case_conv_wgrad_patch's inputs: dW and db of the patch-staged weight-gradient kernel (fp32 atomics: 2e-5 across block counts)"""
    out = []
    for Bn, H, W, Ci, Co, stride in ([(4, 256, 256, 32, 64, 1), (4, 512, 512, 32, 32, 2)] if big else [(2, 5, 64, 32, 64, 1), (1, 6, 128, 32, 32, 2)]):
        g = torch.Generator().manual_seed(21)
        x, w = rnd((Bn, Ci, H, W), dev, g), rnd((Co, Ci, 3, 3), dev, g, 1 / math.sqrt(9 * Ci))
        Ho, Wo = (H, W) if stride == 1 else (H // 2, W // 2)
        dy = rnd((Bn, Co, Ho, Wo), dev, g)
        w32 = w.float().clone().requires_grad_(True)               # fp32 torch autograd, as in case_conv_wgrad_patch
        (F.conv2d(x.float(), w32, padding=1) if stride == 1 else F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), w32, stride=2)).backward(dy.float())
        xn = x.permute(0, 2, 3, 1).contiguous().reshape(-1, Ci)
        dyn = dy.permute(0, 2, 3, 1).contiguous().reshape(-1, Co)
        cd, _, _ = K.conv_fwd_desc(H, W, Ci, 3, stride, 1 if stride == 1 else 0, asym_pad=stride == 2)
        dW, db = K.conv_wgrad(dyn, xn, Bn * Ho * Wo, Co, 9 * Ci, cd, with_bias=True)
        tag = f"wgrad {(Bn, H, W, Ci, Co)} stride {stride}"
        out += [(f"{tag} dW", dW, w32.grad.permute(0, 2, 3, 1).reshape(Co, 9 * Ci), 1e-4, False, 2e-5),
                (f"{tag} db", db, dy.float().sum((0, 2, 3)), 1e-4, False, 2e-5)]
    return out


# knob -> (launch set, limit across settings for the launches that are not `exact` (0.0: the same bits on every launch; None: the
# launch's own sixth element), repeat launches give the same bits)
_OPTION_SETS = {"epi_hoist": (_launches_epilogue, 2e-5, True), "epi_two_phase": (_launches_epilogue, 0.0, True),
                "gn_unroll": (_launches_groupnorm, 0.0, True), "gn_blocks": (_launches_groupnorm, None, True),
                "strip_blocks": (_launches_strip, 0.0, True), "wgrad_patch": (_launches_wgrad_patch, None, False)}


def case_option_invariance(dev, name, value, big=None):
    """One row of the option table: the knob's launch set at the default and at `value` -- both agree with the fp64 reference (fp32 torch for
    the convolutions, as in their own cases) inside the family's limits, repeat launches give the same bits at either setting (except the kernels that use atomics), and across the two
    settings the results are bit-identical wherever include/clora.h promises it and inside the stated limit elsewhere:
      "epi_hoist"    orders the four products of the rank-4 adapter term differently: 2e-5 (case_gemm_fused_down) on adapter launches,
                     same bits on launches without an adapter and with lora_dpack (those always hoist);
      "gn_blocks"    re-partitions the fp32 sums of the two-launch GroupNorm plan: 2e-4 / 1e-5 / 3e-4 for y / statistics / dx
                     (case_groupnorm), same bits on the one-launch plans;
      "wgrad_patch"  fp32 atomics in another order: 2e-5 (case_conv_wgrad_patch);
      "epi_two_phase", "gn_unroll", "strip_blocks": same bits everywhere."""
    launches, across, stable = _OPTION_SETS[name]
    big = (dev != "cpu") if big is None else big
    assert value != option_default(name)
    runs = {}
    for setting in (option_default(name), value):
        with options(**{name: setting}):
            runs[setting] = launches(dev, big)
            again = launches(dev, big) if stable else None
        for i, (label, got, ref, lim, *_) in enumerate(runs[setting]):
            if ref is not None:
                e = rel64(got, ref)
                assert e < lim, (name, setting, label, e)
                if lim > 1e-4:
                    no_outliers(got, ref, label)
            if again is not None:
                assert torch.equal(got, again[i][1]), (name, setting, label, "two identical launches differ")
    changed = []
    for (label, a, _, _, exact, *own), (_, b_, *_rest) in zip(runs[option_default(name)], runs[value]):
        if torch.equal(a, b_):
            continue
        e = rel64(b_, a)
        changed.append((label, e))
        lim = 0.0 if exact else (across if across is not None else own[0])   # a knob's own promise (0.0: same bits) beats the launch's
        assert e < lim, (name, value, label, f"differs by {e:.2e} across settings (limit {lim:.0e})")
    print(f"OPTION {name}={value} vs {option_default(name)}: {len(runs[value])} launches, bits changed in {len(changed)}" +
          (f", worst {max(changed, key=lambda c: c[1])}" if changed else ""))
    return changed
