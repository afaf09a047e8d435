// clora_control_chain.hip -- the control adds of a chain of frozen version-2 ControlLoRA processors at one side of an attention site
// (include/clora.h clora_control_chain_f16) as ONE launch.
//
// Every V2 processor i of a chain updates the hidden states in turn (reference models.py:366-372, 412-418):
//   t_i = Dh_i h_{i-1} + Dc_i ctrl_i,   h_i = h_{i-1} + s U_i t_i
// which closes in rank space: Dh_i h_{i-1} = Dh_i h + s sum_{j<i} (Dh_i U_j) t_j.  With the stacked ranks a, b < R <= 32:
//   p[m,a] = sum_k Dh[a,k] float(H[m,k]) + Tc[m % rows_t, a]
//   t[m,a] = p[m,a] + s sum_{b : member(b) < member(a)} G[a,b] t[m,b]
//   Y[m,n] = fp16(float(H[m,n]) + s sum_a U[n,a] t[m,a])
// H is read from memory once and Y written once; the row tile stays in registers in between.  A group of L lanes (8 .. 64, the
// smallest that covers a row in five 16-byte words per lane) owns RS rows: lane l of the group holds columns 8 (l + L p) .. + 8 of
// pass p.  Down-projection: the lane walks its columns in ascending order against Dh rows streamed through L1 / L2 (16-byte loads,
// contiguous over the lanes), then the L partial sums of a (row, rank) meet in a fixed xor butterfly -- every lane of the group ends
// with the same bits.  The forward substitution (at most 32 unknowns) runs redundantly in every lane of the group.  Expand: U is
// staged rank-major in LDS by the whole block (U is [C, r]: read as it lies it would be a strided walk per lane) -- all of it at the
// start of the block where it fits (two rank-4 processors at any SD width), else the columns of one pass at a time between
// barriers -- and each lane reads the 8 columns it owns as two 16-byte words per rank.  All sums are fp32 in a fixed order,
// nothing is rounded before the store, every element is produced by one thread: repeat launches are bit-identical.  A row is read
// completely (all passes) before any of it is written and belongs to one lane group: Y may be H.
#include "clora_common.h"
#include "../../include/clora.h"

namespace {
constexpr int kChainRanks = 32, kChainPasses = 5, kChainMaxLanes = 64;
constexpr int kChainMaxC = kChainMaxLanes * kChainPasses * 8;      // 2560 columns: what five words per lane of a full wave cover
constexpr int kChainLdU = kChainMaxLanes * 8 + 4;                   // fp32 words per rank row of U staged pass by pass: rows stay 16-byte aligned
// fp32 words of LDS for the staged U per rank class.  Up to 8 ranks (two rank-4 processors, the shipped configs) the whole U of a site
// as wide as 1280 fits: it is then staged once, while the row tile is still on its way, instead of pass by pass between barriers
constexpr int chain_whole_cols(int rmax) { return rmax <= 8 ? 1280 : 512; }      // widest C whose whole U is staged, per rank class
constexpr int chain_us_words(int rmax) { return rmax <= 8 ? 8 * (1280 + 4) : rmax * kChainLdU; }

// the job per stacked rank: what the kernel indexes with compile-time rank numbers
struct chain_args_t {
    const half_t* H;
    half_t* Y;
    const float* G;
    int ldh, ldy, ldg, M, C, R, rows_t, lanes;
    int whole;                        // the whole U fits the LDS buffer at row pitch C + 4: staged once
    float scale;
    const float* D[kChainRanks];      // row a of the stacked Dh
    const float* U[kChainRanks];      // column a of the stacked U (element n at U[a][n * ldu[a]])
    const float* T[kChainRanks];      // column a of the stacked Tc (row m at T[a][m * ldt[a]])
    int ldu[kChainRanks], ldt[kChainRanks];
    int first[kChainRanks];           // first stacked rank of a's member: the ranks b < first[a] couple into a
};

// The rank loops walk the ranks four at a time behind one block-uniform branch: the loads of four ranks are in flight together
// (a branch per rank costs a round trip to L2 per rank and pass), and no more than that, so the registers stay bounded.  The host
// points the slots between R and the next multiple of four at the first rank's operands and the staged U rows of those slots are
// zero, so what they compute is multiplied by 0.
template <int RMAX, int RS>
__global__ __launch_bounds__(256) void control_chain_kernel(chain_args_t g) {
    __shared__ __attribute__((aligned(16))) float Us[chain_us_words(RMAX)];     // Us[a][n] (whole), or Us[a][n - n0] of the current pass
    const int L = g.lanes, M = g.M, C = g.C, R = g.R;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & (L - 1), grp = lane / L;
    const int chunks = C >> 3;
    const int m0 = ((blockIdx.x * 4 + wave) * (64 / L) + grp) * RS;             // (the host keeps this below 2^31)
    const float s = g.scale;

    // the row tile: every pass of every row in flight before the first use
    half8 h[RS][kChainPasses];
#pragma unroll
    for (int p = 0; p < kChainPasses; ++p) {
        const int chunk = p * L + li;
#pragma unroll
        for (int r = 0; r < RS; ++r)
            h[r][p] = (chunk < chunks && m0 + r < M) ? ld8(g.H + (size_t)(m0 + r) * g.ldh + chunk * 8) : zero8();
    }
    const bool whole = g.whole != 0;
    const int ldus = whole ? C + 4 : kChainLdU;
    const int R4 = (R + 3) & ~3;
    if (whole) {                                                                // (read after the barrier that precedes the expand)
        for (int a = 0; a < R4; ++a) {
            const float* u = g.U[a];
            const int ldu = g.ldu[a];
            for (int n = threadIdx.x; n < C; n += 256) Us[a * ldus + n] = a < R ? u[(size_t)n * ldu] : 0.f;
        }
    }

    // ---- p = Dh . h: this lane's columns in ascending order
    float t[RS][RMAX];
#pragma unroll
    for (int r = 0; r < RS; ++r)
#pragma unroll
        for (int a = 0; a < RMAX; ++a) t[r][a] = 0.f;
#pragma unroll
    for (int p = 0; p < kChainPasses; ++p) {
        if (p * L < chunks) {                                                   // block-uniform
            const int chunk = p * L + li;
            const int n = chunk < chunks ? chunk * 8 : 0;                       // (a lane past the row holds zeros: any valid address)
#pragma unroll
            for (int a0 = 0; a0 < RMAX; a0 += 4) {
                if (a0 < R) {                                                   // block-uniform
                    floatx4 d0[4], d1[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        d0[i] = *reinterpret_cast<const floatx4*>(g.D[a0 + i] + n);
                        d1[i] = *reinterpret_cast<const floatx4*>(g.D[a0 + i] + n + 4);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
#pragma unroll
                        for (int r = 0; r < RS; ++r) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) t[r][a0 + i] += d0[i][e] * (float)h[r][p][e];
#pragma unroll
                            for (int e = 0; e < 4; ++e) t[r][a0 + i] += d1[i][e] * (float)h[r][p][4 + e];
                        }
                    }
                }
            }
        }
    }
    // the L partial sums of a (row, rank): xor butterfly, the same bits in every lane of the group; then the control map's share
    int trow[RS];
#pragma unroll
    for (int r = 0; r < RS; ++r) trow[r] = (m0 + r < M ? m0 + r : M - 1) % g.rows_t;
#pragma unroll
    for (int a0 = 0; a0 < RMAX; a0 += 4) {
        if (a0 < R) {                                                           // block-uniform: whole waves take the shuffles
#pragma unroll
            for (int a = a0; a < a0 + 4; ++a) {
#pragma unroll
                for (int r = 0; r < RS; ++r) {
                    float v = t[r][a];
                    for (int mask = L >> 1; mask; mask >>= 1) v += __shfl_xor(v, mask);
                    t[r][a] = v + g.T[a][(size_t)trow[r] * g.ldt[a]];
                }
            }
        }
    }
    // ---- forward substitution over the members: t_a = p_a + s sum_{b < first[a]} G[a,b] t_b.  Of G only the blocks below the block
    // diagonal count: what lies elsewhere in a row is fetched with it and dropped
    if (g.G) {                                                                  // (NULL: a single member, nothing couples)
#pragma unroll
        for (int a = 1; a < RMAX; ++a) {
            const int nb = g.first[a];
            if (a < R && nb > 0) {                                              // block-uniform
                const float* grow = g.G + (size_t)a * g.ldg;
                float sum[RS];
#pragma unroll
                for (int r = 0; r < RS; ++r) sum[r] = 0.f;
#pragma unroll
                for (int b = 0; b < a; ++b) {
                    const float gl = grow[b];
                    const float gv = b < nb ? gl : 0.f;
#pragma unroll
                    for (int r = 0; r < RS; ++r) sum[r] += gv * t[r][b];
                }
#pragma unroll
                for (int r = 0; r < RS; ++r) t[r][a] += s * sum[r];
            }
        }
    }
    // ---- expand: Y = fp16(h + s U t), pass by pass
    if (whole) __syncthreads();
#pragma unroll
    for (int p = 0; p < kChainPasses; ++p) {
        if (p * L < chunks) {                                                   // block-uniform: every thread takes the barriers
            const int chunk = p * L + li;
            const int n0 = p * L * 8, ncols = L * 8;
            if (!whole) {                                                       // block-uniform
                __syncthreads();                                                // the previous pass's readers are done
                for (int a = 0; a < R4; ++a) {
                    const float* u = g.U[a];
                    const int ldu = g.ldu[a];
                    for (int nl = threadIdx.x; nl < ncols; nl += 256)
                        Us[a * kChainLdU + nl] = (a < R && n0 + nl < C) ? u[(size_t)(n0 + nl) * ldu] : 0.f;
                }
                __syncthreads();
            }
            const int nu = whole ? (chunk < chunks ? chunk * 8 : 0) : li * 8;   // (a lane past the row stores nothing)
            float out[RS][8];
#pragma unroll
            for (int r = 0; r < RS; ++r)
#pragma unroll
                for (int e = 0; e < 8; ++e) out[r][e] = 0.f;
#pragma unroll
            for (int a0 = 0; a0 < RMAX; a0 += 4) {
                if (a0 < R) {                                                   // block-uniform
#pragma unroll
                    for (int a = a0; a < a0 + 4; ++a) {
                        const floatx4 u0 = *reinterpret_cast<const floatx4*>(Us + a * ldus + nu);
                        const floatx4 u1 = *reinterpret_cast<const floatx4*>(Us + a * ldus + nu + 4);
#pragma unroll
                        for (int r = 0; r < RS; ++r) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) { out[r][e] += u0[e] * t[r][a]; out[r][4 + e] += u1[e] * t[r][a]; }
                        }
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < RS; ++r) {
                if (chunk < chunks && m0 + r < M) {
                    half8 o;
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)h[r][p][e] + s * out[r][e]);
                    st8(g.Y + (size_t)(m0 + r) * g.ldy + chunk * 8, o);
                }
            }
        }
    }
}

template <int RMAX, int RS>
void launch_chain(const chain_args_t& a, hipStream_t stream) {
    const int rows_per_block = 4 * (64 / a.lanes) * RS;
    hipLaunchKernelGGL((control_chain_kernel<RMAX, RS>), dim3((unsigned)clora_cdiv(a.M, rows_per_block)), dim3(256), 0, stream, a);
}
}  // namespace

extern "C" int clora_control_chain_f16(const clora_control_chain_job_t* job, void* stream) {
    if (!job || !job->H || !job->Y || job->M <= 0 || job->C <= 0 || (job->C & 7) || job->C > kChainMaxC || (job->ldh & 7) ||
        (job->ldy & 7) || job->ldh < job->C || job->ldy < job->C || ((uintptr_t)job->H & 15) || ((uintptr_t)job->Y & 15) ||
        job->rows_t <= 0 || job->M % job->rows_t || job->nmem < 1 || job->nmem > CLORA_CONTROL_CHAIN_MAX_MEMBERS)
        return CLORA_ERR_ARG;
    // Y is H itself (same pitch) or a disjoint buffer
    if (!((const void*)job->Y == (const void*)job->H && job->ldy == job->ldh)) {
        const uintptr_t h0 = (uintptr_t)job->H, h1 = h0 + 2 * ((size_t)(job->M - 1) * job->ldh + job->C);
        const uintptr_t y0 = (uintptr_t)job->Y, y1 = y0 + 2 * ((size_t)(job->M - 1) * job->ldy + job->C);
        if (h0 < y1 && y0 < h1) return CLORA_ERR_ARG;
    }
    chain_args_t a;
    a.H = (const half_t*)job->H; a.Y = (half_t*)job->Y; a.G = job->G;
    a.ldh = job->ldh; a.ldy = job->ldy; a.ldg = job->ldg; a.M = job->M; a.C = job->C; a.rows_t = job->rows_t; a.scale = job->scale;
    int R = 0;
    for (int i = 0; i < job->nmem; ++i) {
        const clora_control_chain_member_t& m = job->m[i];
        if (!m.Dh || !m.U || !m.Tc || m.r < 1 || m.r > 16 || R + m.r > kChainRanks || m.ldd < job->C || (m.ldd & 3) ||
            ((uintptr_t)m.Dh & 15) || m.ldu < m.r || m.toff < 0 || m.ldt < m.toff + m.r)
            return CLORA_ERR_ARG;
        for (int j = 0; j < m.r; ++j) {
            a.D[R + j] = m.Dh + (size_t)j * m.ldd;
            a.U[R + j] = m.U + j;
            a.T[R + j] = m.Tc + m.toff + j;
            a.ldu[R + j] = m.ldu;
            a.ldt[R + j] = m.ldt;
            a.first[R + j] = R;
        }
        R += m.r;
    }
    if (job->nmem > 1 && (!job->G || job->ldg < R)) return CLORA_ERR_ARG;
    for (int c = R; c < kChainRanks; ++c) {          // slots past R: valid addresses whose share is multiplied by 0 (see the kernel)
        a.D[c] = a.D[0]; a.U[c] = a.U[0]; a.T[c] = a.T[0];
        a.ldu[c] = a.ldu[0]; a.ldt[c] = a.ldt[0]; a.first[c] = 0;
    }
    a.R = R;
    const int chunks = job->C >> 3;
    int L = 8;
    while (L * kChainPasses < chunks) L *= 2;
    a.lanes = L;
    a.whole = job->C <= chain_whole_cols(R <= 8 ? 8 : (R <= 16 ? 16 : 32));
    // rows per lane group: as many as the registers of the rank class allow while the grid still fills the device
    const int rs_max = R <= 8 ? 4 : 2;
    int RS = rs_max;
    while (RS > 1 && clora_cdiv(job->M, 4 * (64 / L) * RS) < 1024) RS >>= 1;
    hipStream_t st = (hipStream_t)stream;
    if (R <= 8) {
        if (RS == 4) launch_chain<8, 4>(a, st);
        else if (RS == 2) launch_chain<8, 2>(a, st);
        else launch_chain<8, 1>(a, st);
    } else if (R <= 16) {
        if (RS == 2) launch_chain<16, 2>(a, st);
        else launch_chain<16, 1>(a, st);
    } else {
        if (RS == 2) launch_chain<32, 2>(a, st);
        else launch_chain<32, 1>(a, st);
    }
    return clora_check_launch();
}
