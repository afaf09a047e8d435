// clora_control_mix.hip -- the control share of frozen ControlLoRA members chained onto a v1 site (include/clora.h
// clora_control_mix_q_f16).
//
// A frozen control member's q adapter reads h + c_m; its share over h rides in the folded weights (clora_lora_fold_f16), what is left,
// s^2 U_qm t_m, depends on the member's guide alone: t_m [Mc, r] stays in rank space over the whole sampler loop and is added to the q
// block of the projection output here:
//   Y[m, n] = fp16(float(Y[m, n]) + sum_i scale_i * sum_j T_i[m % rows_t, toff_i + j] * U_i[n, j])
// A read-modify-write of M x N fp16, memory bound: at most 32 fp32 FMAs per element against 4 bytes of traffic.  A block owns 64
// columns and walks 128-row chunks; the U rows of its columns are staged in LDS once (rank-major, so a thread reads the 8 columns it
// owns as two 16-byte words), the T rows of a chunk once per chunk (read as broadcasts by the 8 threads of a row).  A thread owns 8
// consecutive columns of 4 rows: 16-byte loads / stores of Y, the four loads in flight before the rank loop starts.  Every element is
// produced by one thread in a fixed order: no atomics, repeat launches are bit-identical.
#include "clora_common.h"
#include "../../include/clora.h"

namespace {
constexpr int kMixCols = 64, kMixRows = 128, kMixRanks = 32;
constexpr int kMixLdU = kMixCols + 4;        // fp32 words per rank row of U: rows stay 16-byte aligned
constexpr int kMixLdT = kMixRanks + 1;       // odd pitch: the 8 rows a wave reads per instruction fall on different banks

__global__ __launch_bounds__(256) void control_mix_kernel(clora_control_mix_job_t job) {
    __shared__ __attribute__((aligned(16))) float Us[kMixRanks * kMixLdU];      // Us[c][n - n0], c = rank index over all members
    __shared__ float Ts[kMixRows * kMixLdT];                                    // Ts[m - m0][c]
    half_t* Y = (half_t*)job.Y;
    const int M = job.M, N = job.N, nmem = job.nmem;
    const int n0 = blockIdx.x * kMixCols;
    const int tc = threadIdx.x & 7, tr = threadIdx.x >> 3;
    const int n = n0 + tc * 8;

    // (the members' ranks sum to at most kMixRanks: checked by the host)
    for (int i = 0, c0 = 0; i < nmem; c0 += job.m[i].r, ++i) {   // U of this block's columns, once
        const clora_control_mix_member_t& a = job.m[i];
        for (int idx = threadIdx.x; idx < kMixCols * a.r; idx += 256) {
            const int nl = idx / a.r, j = idx - nl * a.r;
            Us[(c0 + j) * kMixLdU + nl] = (n0 + nl < N) ? a.U[(size_t)(n0 + nl) * a.ldu + j] : 0.f;
        }
    }
    const int chunks = (M + kMixRows - 1) / kMixRows;
    for (int ch = blockIdx.y; ch < chunks; ch += gridDim.y) { // block-uniform trip count: every thread takes the barriers
        const int m0 = ch * kMixRows;
        __syncthreads();                                      // the previous chunk's readers are done (first pass: nothing to wait for)
        for (int i = 0, c0 = 0; i < nmem; c0 += job.m[i].r, ++i) {
            const clora_control_mix_member_t& a = job.m[i];
            for (int idx = threadIdx.x; idx < kMixRows * a.r; idx += 256) {
                const int ml = idx / a.r, j = idx - ml * a.r;
                const int m = m0 + ml;
                Ts[ml * kMixLdT + c0 + j] = (m < M) ? a.T[(size_t)(m % job.rows_t) * a.ldt + a.toff + j] : 0.f;
            }
        }
        __syncthreads();
        const bool col_ok = n < N;                            // N % 8 == 0: a chunk of 8 columns is all-valid or all-out
        half8 y[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int m = m0 + tr + 32 * h;
            y[h] = (col_ok && m < M) ? ld8(Y + (size_t)m * job.ldy + n) : zero8();
        }
        float acc[4][8];
#pragma unroll
        for (int h = 0; h < 4; ++h)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[h][e] = 0.f;
        for (int i = 0, c0 = 0; i < nmem; c0 += job.m[i].r, ++i) {
            float part[4][8];
#pragma unroll
            for (int h = 0; h < 4; ++h)
#pragma unroll
                for (int e = 0; e < 8; ++e) part[h][e] = 0.f;
            for (int c = c0; c < c0 + job.m[i].r; ++c) {
                const floatx4 u0 = *reinterpret_cast<const floatx4*>(Us + c * kMixLdU + tc * 8);
                const floatx4 u1 = *reinterpret_cast<const floatx4*>(Us + c * kMixLdU + tc * 8 + 4);
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    const float t = Ts[(tr + 32 * h) * kMixLdT + c];
#pragma unroll
                    for (int e = 0; e < 4; ++e) { part[h][e] += t * u0[e]; part[h][4 + e] += t * u1[e]; }
                }
            }
            const float s = job.m[i].scale;
#pragma unroll
            for (int h = 0; h < 4; ++h)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[h][e] += s * part[h][e];
        }
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int m = m0 + tr + 32 * h;
            if (col_ok && m < M) {
                half8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)y[h][e] + acc[h][e]);
                st8(Y + (size_t)m * job.ldy + n, o);
            }
        }
    }
}
}  // namespace

extern "C" int clora_control_mix_q_f16(const clora_control_mix_job_t* job, void* stream) {
    if (!job || !job->Y || job->M <= 0 || job->N <= 0 || (job->N & 7) || (job->ldy & 7) || job->ldy < job->N ||
        ((uintptr_t)job->Y & 15) || job->rows_t <= 0 || job->M % job->rows_t || job->nmem < 1 ||
        job->nmem > CLORA_CONTROL_MIX_MAX_MEMBERS)
        return CLORA_ERR_ARG;
    int ranks = 0;
    for (int i = 0; i < job->nmem; ++i) {
        const clora_control_mix_member_t& a = job->m[i];
        if (!a.T || !a.U || a.r < 1 || a.r > 16 || a.toff < 0 || a.ldt < a.toff + a.r || a.ldu < a.r) return CLORA_ERR_ARG;
        ranks += a.r;
    }
    if (ranks > kMixRanks) return CLORA_ERR_ARG;
    // enough blocks to keep every CU streaming (about 8 per CU), each walking its share of the 128-row chunks
    const int bx = clora_cdiv(job->N, kMixCols), chunks = clora_cdiv(job->M, kMixRows);
    int by = clora_cdiv(2048, bx);
    if (by > chunks) by = chunks;
    if (by > 65535) by = 65535;
    hipLaunchKernelGGL(control_mix_kernel, dim3((unsigned)bx, (unsigned)by), dim3(256), 0, (hipStream_t)stream, *job);
    return clora_check_launch();
}
