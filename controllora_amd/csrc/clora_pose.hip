// clora_pose.hip -- the kernels of the OpenPose body network (controllora_amd/openpose.py; reference annotator/openpose/model.py
// `bodypose_model`): a VGG front of 3x3 convolutions with ReLU and 2x2 max pools, then six stages of two branches each whose
// work is fifty 7x7 convolutions of 128 channels on the 1/8-resolution map -- at the pose app's default 23 x 23 = 529 pixels:
// M = 529, N = 128, K = 49 * 128 = 6272, a deep-K, tiny-M problem that fills a 256-CU chip only if the launch is shaped for it.
//
//   conv_act   stride-1 "same" convolution, ksize 1 / 3 / 7, fp16 NHWC rows in, fp32 accumulation on v_mfma_f32_16x16x32_f16,
//              + bias[n], optional ReLU, fp16 out.  One launch takes the L1 and the L2 branch of a stage as two JOBS (grid.z).
//              A workgroup owns an 8 x 8 pixel tile (four MFMA row fragments of 2 rows x 8 columns) and 64 output channels (one
//              16-wide fragment per wave).  K runs over UNITS (32-channel slab, kernel row ky): per slab the tile's input patch
//              with its ksize/2-pixel halo is staged once in LDS (zero outside the image and past Cin), and per unit the wave
//              walks kx: one 16-byte weight fragment per lane straight from the packed weights (each wave reads other channels,
//              so nothing would be shared through LDS), four LDS patch fragments, four MFMAs.
//              Where pixel tiles x channel tiles x jobs is below the CU count the units are cut into `splits` contiguous ranges
//              (grid.y): every range writes its raw fp32 sums into its own slab of the caller's workspace and a finish launch
//              adds the slabs in a fixed order, then bias / ReLU / rounding.  No atomics: repeat launches give the same bits.
//              Stores write the channels below Cout and nothing else: the branch heads (Cout 38 and 19) store straight into the
//              192-channel stage buffer at channel offsets 128 and 166, which is how the network's concatenation is never copied.
//   pack       OIHW fp32 weights -> the fp16 operand [tap][Cin32 / 8][CoutP][8] with an input-channel permutation / pad table
//   maxpool    2 x 2, stride 2, NHWC fp16, 8 channels per thread
#include "clora_common.h"
#include "../../include/clora.h"

namespace {

constexpr int kTH = 8, kTW = 8;            // output pixel tile
constexpr int kBN = 64;                    // output channels per workgroup: wave w owns channels 16 w .. 16 w + 15 of them
constexpr int kKC = 32;                    // channels per K slab = the k of one MFMA
constexpr int kPS = 40;                    // LDS halves per patch pixel: 32 + 8 pad (80-byte pitch: 16-byte aligned, off the 64-byte bank period)

struct ConvActJob {
    const half_t* x;
    const half_t* w;
    const float* bias;
    half_t* y;
    int ldx, ldy, Cin, Cout, relu;
};

struct ConvActArgs {
    ConvActJob job[CLORA_CONV_ACT_MAX_JOBS];
    float* ws;                             // split-K slabs [job][split][B * H * W][wsN] (splits > 1)
    int B, H, W, tiles_x, tiles_y, ctiles, splits, wsN;
};

__device__ __forceinline__ float activate(float v, int relu) { return relu ? fmaxf(v, 0.f) : v; }

// channels (co, co + 1), co even, of one output row: exactly the channels below Cout are written
__device__ __forceinline__ void store_pair(half_t* yrow, int co, int Cout, float v0, float v1) {
    if (co + 1 < Cout) {
        half2v h = {(half_t)v0, (half_t)v1};
        *reinterpret_cast<half2v*>(yrow + co) = h;
    } else if (co < Cout) {
        yrow[co] = (half_t)v0;
    }
}

template <int KS>
__global__ __launch_bounds__(256) void conv_act_kernel(ConvActArgs P) {
    constexpr int HALO = KS / 2, PH = kTH + 2 * HALO, PW = kTW + 2 * HALO;
    __shared__ __attribute__((aligned(16))) half_t patch[PH * PW * kPS];
    const ConvActJob& J = P.job[blockIdx.z];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, r16 = lane & 15;
    const int ct = blockIdx.y % P.ctiles, split = blockIdx.y / P.ctiles;
    const int CoutP = (J.Cout + 15) & ~15;
    if (ct * kBN >= CoutP) return;                                       // uniform: the other job is the wider one
    const int pt = blockIdx.x, tx = pt % P.tiles_x, ty = (pt / P.tiles_x) % P.tiles_y, b = pt / (P.tiles_x * P.tiles_y);
    const int x0 = tx * kTW, y0 = ty * kTH;
    const int nslab = (J.Cin + kKC - 1) / kKC, U = nslab * KS;          // K units: (channel slab, kernel row)
    const int per = (U + P.splits - 1) / P.splits;
    const int u0 = split * per, u1 = u0 + per < U ? u0 + per : U;       // may be empty: the slab is still written (zeros)
    const int nw = ct * kBN + wave * 16;
    const bool live = nw < CoutP;                                        // wave-uniform
    const half_t* wl = J.w + ((size_t)g * CoutP + nw + r16) * 8;         // this lane's 8 k-slots of its channel, tap 0, slab 0
    floatx4 acc[4] = {zero4f(), zero4f(), zero4f(), zero4f()};
    int staged = -1;
    for (int u = u0; u < u1; ++u) {
        const int slab = u / KS, ky = u - slab * KS;
        if (slab != staged) {
            __syncthreads();                                             // every wave is done with the patch of the slab before
            for (int i = tid; i < PH * PW * 4; i += 256) {
                const int pix = i >> 2, c = i & 3, py = pix / PW, px = pix - py * PW;
                const int y = y0 + py - HALO, x = x0 + px - HALO, ci = slab * kKC + c * 8;
                half8 v = zero8();
                if (y >= 0 && y < P.H && x >= 0 && x < P.W && ci < J.Cin) v = ld8(J.x + ((size_t)(b * P.H + y) * P.W + x) * J.ldx + ci);
                st8(patch + pix * kPS + c * 8, v);
            }
            __syncthreads();
            staged = slab;
        }
        if (!live) continue;
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
            const half8 bv = ld8(wl + (size_t)((ky * KS + kx) * nslab + slab) * 4 * CoutP * 8);
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const half_t* ap = patch + ((2 * f + (r16 >> 3) + ky) * PW + (r16 & 7) + kx) * kPS + g * 8;
                acc[f] = mfma16(ld8(ap), bv, acc[f]);
            }
        }
    }
    if (!live) return;
    const int co = nw + r16;
    const float bias_v = co < J.Cout ? J.bias[co] : 0.f;
    const size_t M = (size_t)P.B * P.H * P.W;
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = 4 * g + r, y = y0 + 2 * f + (p >> 3), x = x0 + (p & 7);
            const bool in = y < P.H && x < P.W;
            const size_t row = (size_t)(b * P.H + y) * P.W + x;
            if (P.splits > 1) {
                const float part = acc[f][r];                            // raw sums: bias and activation belong to the finish pass
                if (in) P.ws[((size_t)(blockIdx.z * P.splits + split) * M + row) * P.wsN + co] = part;
            } else {
                const float v = activate(acc[f][r] + bias_v, J.relu);
                const float right = __shfl_xor(v, 1);                    // the odd neighbour's channel: one 4-byte store per pair
                if (in && (lane & 1) == 0) store_pair(J.y + row * J.ldy, co, J.Cout, v, right);
            }
        }
}

// y = act(sum over the slabs in order + bias), one thread per channel pair of a row
__global__ __launch_bounds__(256) void conv_act_finish_kernel(ConvActArgs P) {
    const ConvActJob& J = P.job[blockIdx.y];
    const size_t M = (size_t)P.B * P.H * P.W, pairs = (size_t)(J.Cout + 1) / 2, total = M * pairs;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t row = i / pairs;
        const int co = 2 * (int)(i - row * pairs);
        float v0 = 0.f, v1 = 0.f;
        for (int s = 0; s < P.splits; ++s) {
            const float* p = P.ws + ((size_t)(blockIdx.y * P.splits + s) * M + row) * P.wsN + co;   // co + 1 < CoutP <= wsN
            v0 += p[0];
            v1 += p[1];
        }
        v0 = activate(v0 + J.bias[co], J.relu);
        v1 = activate(v1 + (co + 1 < J.Cout ? J.bias[co + 1] : 0.f), J.relu);
        store_pair(J.y + row * J.ldy, co, J.Cout, v0, v1);
    }
}

__global__ __launch_bounds__(256) void conv_act_pack_kernel(const float* w, half_t* out, const int* perm, int Cout, int CinSrc, int CinDst,
                                                            int ksize, size_t total) {
    const int CoutP = (Cout + 15) & ~15, CS = (CinDst + kKC - 1) / kKC * 4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int e = (int)(i & 7);
        size_t q = i >> 3;
        const int co = (int)(q % CoutP);
        q /= CoutP;
        const int cs = (int)(q % CS), tap = (int)(q / CS), cd = cs * 8 + e;
        int src = -1;
        if (cd < CinDst) src = perm ? perm[cd] : cd;
        float v = 0.f;
        if (co < Cout && src >= 0 && src < CinSrc) v = w[((size_t)co * CinSrc + src) * ksize * ksize + tap];
        out[i] = (half_t)v;
    }
}

__device__ __forceinline__ half_t max_like_torch(half_t m, half_t v) { return (v > m || v != v) ? v : m; }

__global__ __launch_bounds__(256) void maxpool2x2_kernel(const half_t* x, half_t* y, int H, int W, int C, size_t total) {
    const int Ho = H / 2, Wo = W / 2, C8 = C / 8;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % C8);
        size_t q = i / C8;
        const int xo = (int)(q % Wo);
        q /= Wo;
        const int yo = (int)(q % Ho);
        const size_t b = q / Ho;
        const half_t* p = x + (((b * H + 2 * yo) * W + 2 * xo) * C) + c * 8;
        half8 m = ld8(p);                                                // F.max_pool2d's scan order: (0,0) (0,1) (1,0) (1,1)
        const half8 v1 = ld8(p + C), v2 = ld8(p + (size_t)W * C), v3 = ld8(p + (size_t)W * C + C);
        for (int e = 0; e < 8; ++e) m[e] = max_like_torch(max_like_torch(max_like_torch(m[e], v1[e]), v2[e]), v3[e]);
        st8(y + i * 8, m);
    }
}

struct ConvActPlan {
    int tiles_x, tiles_y, ptiles, ctiles, splits, wsN;
};

// the launch shape, a function of the problem alone (never of a knob): repeat calls take the same path and give the same bits
bool conv_act_plan(const clora_conv_act_job_t* jobs, int njobs, int B, int H, int W, int ksize, ConvActPlan& pl) {
    if (!jobs || njobs < 1 || njobs > CLORA_CONV_ACT_MAX_JOBS || B <= 0 || H <= 0 || W <= 0) return false;
    if (ksize != 1 && ksize != 3 && ksize != 7) return false;
    if ((long)B * H * W > 0x7fffffffL) return false;
    int max_cout = 0, max_units = 0;
    for (int j = 0; j < njobs; ++j) {
        const clora_conv_act_job_t& q = jobs[j];
        if (!q.x || !q.w || !q.bias || !q.y || q.Cin <= 0 || q.Cin % 8 != 0 || q.Cout <= 0) return false;
        if (q.ldx < q.Cin || q.ldx % 8 != 0 || ((uintptr_t)q.x & 15) != 0 || ((uintptr_t)q.w & 15) != 0) return false;
        if (q.ldy < q.Cout || q.ldy % 2 != 0 || ((uintptr_t)q.y & 3) != 0) return false;      // an odd channel offset lands here
        max_cout = q.Cout > max_cout ? q.Cout : max_cout;
        const int units = (q.Cin + kKC - 1) / kKC * ksize;
        max_units = units > max_units ? units : max_units;
    }
    pl.tiles_x = clora_cdiv(W, kTW);
    pl.tiles_y = clora_cdiv(H, kTH);
    const long ptiles = (long)B * pl.tiles_x * pl.tiles_y;
    if (ptiles > 0x7fffffffL) return false;
    pl.ptiles = (int)ptiles;
    pl.wsN = (max_cout + 15) & ~15;
    pl.ctiles = clora_cdiv(pl.wsN, kBN);
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        cus = 256;
    const long base = ptiles * pl.ctiles * njobs;
    pl.splits = 1;
    if (base < cus) {
        int want = clora_cdiv(cus, base);
        want = want < max_units ? want : max_units;
        const int per = clora_cdiv(max_units, want);
        pl.splits = clora_cdiv(max_units, per);                          // no empty range for the job with the most units
    }
    if ((long)pl.ctiles * pl.splits > 65535) return false;
    return true;
}

size_t conv_act_ws_bytes(const ConvActPlan& pl, int njobs, int B, int H, int W) {
    return pl.splits > 1 ? (size_t)njobs * pl.splits * B * H * W * pl.wsN * sizeof(float) : 0;
}

}  // namespace

extern "C" int clora_conv_act_splits(const clora_conv_act_job_t* jobs, int njobs, int B, int H, int W, int ksize) {
    ConvActPlan pl;
    return conv_act_plan(jobs, njobs, B, H, W, ksize, pl) ? pl.splits : CLORA_ERR_ARG;
}

extern "C" size_t clora_conv_act_workspace(const clora_conv_act_job_t* jobs, int njobs, int B, int H, int W, int ksize) {
    ConvActPlan pl;
    return conv_act_plan(jobs, njobs, B, H, W, ksize, pl) ? conv_act_ws_bytes(pl, njobs, B, H, W) : 0;
}

extern "C" int clora_conv_act_f16(const clora_conv_act_job_t* jobs, int njobs, int B, int H, int W, int ksize, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    ConvActPlan pl;
    if (!conv_act_plan(jobs, njobs, B, H, W, ksize, pl)) return CLORA_ERR_ARG;
    const size_t need = conv_act_ws_bytes(pl, njobs, B, H, W);
    if (need > 0 && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15) != 0)) return CLORA_ERR_WORKSPACE;
    ConvActArgs A = {};
    for (int j = 0; j < njobs; ++j) {
        const clora_conv_act_job_t& q = jobs[j];
        A.job[j] = ConvActJob{(const half_t*)q.x, (const half_t*)q.w, q.bias, (half_t*)q.y, q.ldx, q.ldy, q.Cin, q.Cout, q.relu};
    }
    A.ws = (float*)workspace;
    A.B = B, A.H = H, A.W = W, A.tiles_x = pl.tiles_x, A.tiles_y = pl.tiles_y, A.ctiles = pl.ctiles, A.splits = pl.splits, A.wsN = pl.wsN;
    const dim3 grid(pl.ptiles, pl.ctiles * pl.splits, njobs);
    if (ksize == 7)
        hipLaunchKernelGGL(conv_act_kernel<7>, grid, dim3(256), 0, (hipStream_t)stream, A);
    else if (ksize == 3)
        hipLaunchKernelGGL(conv_act_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, A);
    else
        hipLaunchKernelGGL(conv_act_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, A);
    if (pl.splits > 1) {
        const size_t work = (size_t)B * H * W * ((pl.wsN + 1) / 2), blocks = (work + 255) / 256;
        hipLaunchKernelGGL(conv_act_finish_kernel, dim3((unsigned)(blocks > 2048 ? 2048 : blocks), njobs), dim3(256), 0, (hipStream_t)stream, A);
    }
    return clora_check_launch();
}

extern "C" int clora_conv_act_pack_f32(const float* w, clora_half* out, const int* perm, int Cout, int CinSrc, int CinDst, int ksize,
                                       void* stream) {
    if (!w || !out || Cout <= 0 || CinSrc <= 0 || CinDst <= 0 || CinDst % 8 != 0 || (ksize != 1 && ksize != 3 && ksize != 7)) return CLORA_ERR_ARG;
    const size_t total = (size_t)ksize * ksize * ((CinDst + kKC - 1) / kKC * kKC) * ((Cout + 15) & ~15), blocks = (total + 255) / 256;
    hipLaunchKernelGGL(conv_act_pack_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, (hipStream_t)stream, w,
                       (half_t*)out, perm, Cout, CinSrc, CinDst, ksize, total);
    return clora_check_launch();
}

extern "C" int clora_maxpool2x2_f16(const clora_half* x, clora_half* y, int B, int H, int W, int C, void* stream) {
    if (!x || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0 || H % 2 != 0 || W % 2 != 0 || C % 8 != 0) return CLORA_ERR_ARG;
    if ((((uintptr_t)x | (uintptr_t)y) & 15) != 0) return CLORA_ERR_ARG;
    const size_t total = (size_t)B * (H / 2) * (W / 2) * (C / 8), blocks = (total + 255) / 256;
    hipLaunchKernelGGL(maxpool2x2_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)x, (half_t*)y, H, W, C, total);
    return clora_check_launch();
}
