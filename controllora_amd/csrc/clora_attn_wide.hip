// clora_attn_wide.hip -- forward flash attention for head dims 160 < D <= 512 on gfx950.
//
// The one user is the VAE's mid-block attention (controllora_amd/vae.py: a single head of 512 channels over every latent
// token; 9,216 tokens for a 768 x 768 image), which used to materialise its N x N scores.  Same contract and same
// register-level design as the forward of clora_attn.hip (transposed scores S^T = K . Q^T so the softmax statistics are
// lane-local, lazy exponent reference, C-layout tile fed back as the B operand, LDS-DMA double-buffered K / V tiles);
// what changes is the budget.  One instantiation, padded to 512 along the contraction and the output dim:
//   * registers: a wave owns QG groups of 16 queries.  Per group the Q fragments are 16 k-steps x 4 = 64 VGPRs and the
//     O^T accumulators 32 d-tiles x 4 = 128.  QG = 1 fits the 256-register step (two waves per SIMD, 8 waves = 128
//     queries per block) and is the one instantiation.  QG = 2 (the whole 512-register file, one wave per SIMD, 4 waves
//     per block; every K / V fragment read from LDS once for two query groups) was compiled and dropped on the
//     compiler's report, before any timing: 326 VGPRs spilled to scratch and ~600 v_accvgpr moves plus ~70 scratch
//     loads per key tile against 128 MFMAs (QG = 1: 26 spilled, 5 scratch loads per tile, no accumulator moves) --
//     the one-wave-per-SIMD regime that lost 15-50 % on the GEMM / conv loops.
//   * LDS: a 32-key tile at pitch 512 + 16 halves is 33,792 B; K + V double-buffered is 135,168 B of the CU's 163,840:
//     one block per CU.  32 keys is the smallest tile the C-layout feedback allows (two 16-key score tiles make the
//     8 k-slots of the P operand).
//   * the K . Q^T chain of a query group is 16 dependent MFMAs per 16-key tile; with QG = 1 it is split into two
//     partial accumulators (even / odd k-steps) so four independent chains are in flight per wave.
// No backward: the VAE is frozen (clora_attn_bwd_f16 keeps its limit of 160).
#include "clora_attn_common.h"
#include "../../include/clora.h"

namespace {

template <int QG, int NWV>
__global__ __launch_bounds__(NWV * 64, 1) void attn_fwd_wide_kernel(AttnArgs p) {
    constexpr int DP = 512, BKV = 32, LD = DP + 16, KS = DP / 32, DT = DP / 16, QW = QG * 16, SP = QG == 1 ? 2 : 1;
    constexpr int TILE = 2 * BKV * LD;                     // one K tile + one V tile; two of them: double buffer
    __shared__ __attribute__((aligned(16))) half_t smem[2 * TILE];
    const int t = threadIdx.x, w = t >> 6, l = t & 63, g = l >> 4, li = l & 15;
    int bx, by;
    attn_block_ids(p, bx, by);
    const int b = by / p.H, h = by % p.H;
    const int q0 = bx * (NWV * QW) + w * QW;
    const int D = p.D;
    const float c = p.scale * kLog2e;

    const half_t* kbase = p.k + (size_t)b * p.Nk * p.ldk + h * D;
    const half_t* vbase = p.v + (size_t)b * p.Nk * p.ldv + h * D;
    TileDma<BKV, LD, NWV> dma;                             // K and V tiles share the slot -> (row, column) map
    dma.init(w, l, D);
    {
        const int rows0 = p.Nk < BKV ? p.Nk : BKV;
        dma.template issue<false>(kbase, p.ldk, rows0, smem, w);
        dma.template issue<false>(vbase, p.ldv, rows0, smem + BKV * LD, w);
    }

    half8 qf[QG][KS];      // Q pre-multiplied by scale*log2(e): scores come out of the MFMA ready for exp2
#pragma unroll
    for (int qg = 0; qg < QG; ++qg)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int q = q0 + qg * 16 + li, d = ks * 32 + g * 8;
            half8 v = (q < p.Nq && d < D) ? ld8(p.q + ((size_t)b * p.Nq + q) * p.ldq + h * D + d) : zero8();
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (half_t)((float)v[e] * c);
            qf[qg][ks] = v;
        }
    floatx4 oacc[DT][QG];
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int qg = 0; qg < QG; ++qg) oacc[i][qg] = zero4f();
    float mref[QG], lrun[QG];
#pragma unroll
    for (int qg = 0; qg < QG; ++qg) { mref[qg] = 0.f; lrun[qg] = 0.f; }
    bool first = true;

    CLORA_WAIT_VMCNT(0);
    __syncthreads();                                       // tile 0 has landed for every wave
    int cur = 0;
    for (int kv0 = 0; kv0 < p.Nk; kv0 += BKV) {
        const int rows = (p.Nk - kv0 < BKV) ? p.Nk - kv0 : BKV;
        const half_t* Ks = smem + cur * TILE;
        const half_t* Vs = Ks + BKV * LD;                  // V row-major [key][d]; read transposed (frag_tr) for P.V
        if (kv0 + BKV < p.Nk) {                            // tile t+1 -> the other buffer (consumed in iteration t-1, barrier since)
            const int nrows = (p.Nk - kv0 - BKV < BKV) ? p.Nk - kv0 - BKV : BKV;
            half_t* nb = smem + (cur ^ 1) * TILE;
            dma.template issue<false>(kbase + (size_t)(kv0 + BKV) * p.ldk, p.ldk, nrows, nb, w);
            dma.template issue<false>(vbase + (size_t)(kv0 + BKV) * p.ldv, p.ldv, nrows, nb + BKV * LD, w);
        }

        floatx4 s[2][QG], s2[2][QG];                       // s2: the odd k-steps' partial sums (SP == 2)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int qg = 0; qg < QG; ++qg) { s[kt][qg] = splat4f(-mref[qg]); s2[kt][qg] = zero4f(); }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                const half8 a = ld8(Ks + (kt * 16 + li) * LD + ks * 32 + g * 8);
#pragma unroll
                for (int qg = 0; qg < QG; ++qg) {
                    if (SP == 2 && (ks & 1)) s2[kt][qg] = mfma16(a, qf[qg][ks], s2[kt][qg]);
                    else s[kt][qg] = mfma16(a, qf[qg][ks], s[kt][qg]);
                }
            }
        if (SP == 2) {
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int qg = 0; qg < QG; ++qg) s[kt][qg] += s2[kt][qg];
        }
        if (rows < BKV) {                                  // ragged last tile only: mask the missing keys
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (kt * 16 + 4 * g + r >= rows) {
#pragma unroll
                        for (int qg = 0; qg < QG; ++qg) s[kt][qg][r] = kNegBig;
                    }
        }
        float mx[QG];
        bool rebase = first;
#pragma unroll
        for (int qg = 0; qg < QG; ++qg) {
            float m = kNegBig;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) m = fmaxf(m, s[kt][qg][r]);
            m = fmaxf(m, __shfl_xor(m, 16));
            m = fmaxf(m, __shfl_xor(m, 32));
            mx[qg] = m;                                    // tile maximum relative to mref, same in the 4 lanes of a query
            rebase = rebase || m > kRebase;
        }
        if (__any(rebase)) {
#pragma unroll
            for (int qg = 0; qg < QG; ++qg) {
                const float d = (first || mx[qg] > kRebase) ? mx[qg] : 0.f;
                // first tile: O and l are still zero and d may be hugely negative (every logit of the tile below -88:
                // exp2(-d) = +inf and 0 * inf = NaN) -- nothing to rescale yet
                const float alpha = first ? 1.f : CLORA_EXP2(-d);
                mref[qg] += d;
                lrun[qg] *= alpha;
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) s[kt][qg] -= d;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) oacc[dt][qg] *= alpha;
            }
            first = false;
        }
        half8 pb[QG];
#pragma unroll
        for (int qg = 0; qg < QG; ++qg) {
            float ps = 0.f;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pv = CLORA_EXP2(s[kt][qg][r]);
                    s[kt][qg][r] = pv;
                    ps += pv;
                }
            lrun[qg] += ps;
            pb[qg] = frag_from_acc(s[0][qg], s[1][qg]);
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const half8 a = frag_tr<LD>(Vs, dt * 16, 0, g, l);
#pragma unroll
            for (int qg = 0; qg < QG; ++qg) oacc[dt][qg] = mfma16(a, pb[qg], oacc[dt][qg]);
        }
        CLORA_WAIT_VMCNT(0);                               // this wave's share of tile t+1 has landed ...
        __syncthreads();                                   // ... everyone's has, and tile t is fully consumed
        cur ^= 1;
    }
#pragma unroll
    for (int qg = 0; qg < QG; ++qg) {
        float lt = lrun[qg];
        lt += __shfl_xor(lt, 16);
        lt += __shfl_xor(lt, 32);
        const float inv = 1.0f / lt;
        const int q = q0 + qg * 16 + li;
        if (q < p.Nq) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const int d = dt * 16 + 4 * g;
                if (d < D) {
                    half4v o;
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = (half_t)(oacc[dt][qg][r] * inv);
                    st4(p.out + ((size_t)b * p.Nq + q) * p.ldo + h * D + d, o);
                }
            }
            if (g == 0 && p.lse) p.lse[((size_t)b * p.H + h) * p.Nq + q] = (mref[qg] + log2f(lt)) * kLn2;
        }
    }
}

}  // namespace

int clora_attn_fwd_wide(const AttnArgs& a, hipStream_t s) {
    if (a.D <= 160 || a.D > 512) return CLORA_ERR_ARG;
    const dim3 grid(clora_cdiv(a.Nq, 128), a.B * a.H);
    hipLaunchKernelGGL((attn_fwd_wide_kernel<1, 8>), grid, dim3(512), 0, s, a);
    return clora_check_launch();
}
