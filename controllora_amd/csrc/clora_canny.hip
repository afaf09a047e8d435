// clora_canny.hip -- the Canny edge detector of the `process/diffusiondb_canny` data path and of apps/canny2image.py on the
// device.  The numpy detector `controllora_amd.process.canny` is the specification; three kernels:
//
//   classify   uint8 [B,H,W,C] image (C = 3 RGB or 1 grey) + per-image thresholds -> uint8 [B,H,W] class map
//              (0 = no candidate, 1 = weak, 2 = strong).  One launch per batch.  A workgroup stages its 64x16 tile plus a
//              2-pixel halo once in LDS as fp32 grey (Sobel reads 1 pixel around, the suppression reads the magnitude of the
//              8 neighbours, hence 2), then grey -> Sobel -> L1 magnitude -> sector -> suppression -> class without going
//              back to memory.  Borders as in numpy: grey edge-replicated for Sobel, magnitude zero-padded for suppression.
//              Every fp32 operation is rounded on its own and summed in numpy's order (contraction off), so grey, gx, gy and
//              the magnitude are the numpy values bit for bit.  The sector is NOT numpy's fp32 atan2: it is found by comparing
//              |gy| with tan(22.5 deg) |gx| and tan(67.5 deg) |gx| in fp64, i.e. exact to ~1e-14 deg; numpy's own answer is
//              rounding noise within ~2e-5 deg of a sector boundary and the two may differ only there.
//   hysteresis one pass over a state map (a copy of the class map that is updated in place, 1 -> 2): a workgroup loads its
//              64x32 tile plus a 1-pixel halo into LDS, grows strong through weak until the tile is stable, stores the pixels
//              that turned strong and raises the pass's "changed" word.  Passes repeat until a pass changes nothing; the fixed
//              point is unique, so neither the order of growth inside a pass nor a neighbour tile's concurrent update of a halo
//              byte (monotone 1 -> 2, byte stores) can change the result.  The export enqueues a GROUP of passes; every pass
//              returns at once when the word of the pass before it is zero, so the host reads one word back per group and
//              nothing ever waits for another workgroup inside a launch.
//   emit       state map -> uint8 {0, 255} edge map and / or the trainer's guide tensor fp16 [B,3,H,W] in {-1, +1}.
#include "clora_common.h"
#include "../../include/clora.h"

namespace {

constexpr int kCW = 64, kCH = 16;          // classify tile (256 threads, 4 pixels each)
constexpr int kHW = 64, kHH = 32;          // hysteresis tile (256 threads, a run of 8 pixels each)
constexpr int kHS = kHW + 4;               // LDS row stride of the hysteresis tile (66 used)

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// numpy: 0.299 * R + 0.587 * G + 0.114 * B on float32 arrays = ((0.299f R) + (0.587f G)) + (0.114f B), four roundings
__device__ __forceinline__ float grey_of(float r, float g, float b) {
#pragma clang fp contract(off)
    const float pr = 0.299f * r;
    const float pg = 0.587f * g;
    const float pb = 0.114f * b;
    const float s = pr + pg;
    return s + pb;
}

// gradient direction folded to [0, 180) and binned at 22.5 / 67.5 / 112.5 / 157.5 degrees: 0 = E-W, 1 = NE-SW (gx, gy of equal
// sign), 2 = N-S, 3 = NW-SE.  gx = gy = 0 is sector 0 like numpy's atan2(0, 0) = 0.
__device__ __forceinline__ int sector_of(float gx, float gy) {
#pragma clang fp contract(off)
    const double ax = fabs((double)gx), ay = fabs((double)gy);
    const double t1 = 0.41421356237309503 * ax;      // tan(22.5 deg)
    const double t2 = 2.414213562373095 * ax;        // tan(67.5 deg)
    if (ay <= t1) return 0;
    if (ay >= t2) return 2;
    return ((gx > 0.f) == (gy > 0.f)) ? 1 : 3;
}

__global__ __launch_bounds__(256) void canny_classify_kernel(const uint8_t* img, const float* low, const float* high, uint8_t* cls,
                                                             int H, int W, int C) {
    __shared__ float grey[kCH + 4][kCW + 4];
    __shared__ float mag[kCH + 2][kCW + 2];
    __shared__ uint8_t sec[kCH + 2][kCW + 2];
    const int b = blockIdx.z, x0 = blockIdx.x * kCW, y0 = blockIdx.y * kCH, tid = threadIdx.x;
    const uint8_t* src = img + (size_t)b * H * W * C;
    for (int i = tid; i < (kCH + 4) * (kCW + 4); i += 256) {              // grey with the image's edge replicated
        const int ly = i / (kCW + 4), lx = i - ly * (kCW + 4);
        const int y = clampi(y0 + ly - 2, 0, H - 1), x = clampi(x0 + lx - 2, 0, W - 1);
        const uint8_t* p = src + ((size_t)y * W + x) * C;
        grey[ly][lx] = (C == 3) ? grey_of((float)p[0], (float)p[1], (float)p[2]) : (float)p[0];
    }
    __syncthreads();
    for (int i = tid; i < (kCH + 2) * (kCW + 2); i += 256) {              // Sobel, numpy's order of additions; magnitude 0 outside
        const int ly = i / (kCW + 2), lx = i - ly * (kCW + 2);
        const int y = y0 + ly - 1, x = x0 + lx - 1;
        float m = 0.f;
        int s = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
#pragma clang fp contract(off)
            const float a = grey[ly][lx], bb = grey[ly][lx + 1], c = grey[ly][lx + 2];
            const float d = grey[ly + 1][lx], f = grey[ly + 1][lx + 2];
            const float g = grey[ly + 2][lx], h = grey[ly + 2][lx + 1], k = grey[ly + 2][lx + 2];
            float gx = 0.f - a;
            gx = gx + c;
            gx = gx - 2.0f * d;
            gx = gx + 2.0f * f;
            gx = gx - g;
            gx = gx + k;
            float gy = 0.f - a;
            gy = gy - 2.0f * bb;
            gy = gy - c;
            gy = gy + g;
            gy = gy + 2.0f * h;
            gy = gy + k;
            m = fabsf(gx) + fabsf(gy);
            s = sector_of(gx, gy);
        }
        mag[ly][lx] = m;
        sec[ly][lx] = (uint8_t)s;
    }
    __syncthreads();
    const float t0 = low[b], t1 = high[b];
    const float lo = t0 <= t1 ? t0 : t1, hi = t0 <= t1 ? t1 : t0;         // swapped when low > high, as cv2.Canny does
    uint8_t* dst = cls + (size_t)b * H * W;
    for (int i = tid; i < kCH * kCW; i += 256) {
        const int ly = i / kCW, lx = i - ly * kCW;
        const int y = y0 + ly, x = x0 + lx;
        if (y >= H || x >= W) continue;
        const float m = mag[ly + 1][lx + 1];
        const int s = sec[ly + 1][lx + 1];
        const int dy = s == 0 ? 0 : 1, dx = s == 0 ? 1 : (s == 1 ? 1 : (s == 2 ? 0 : -1));
        const float n0 = mag[ly + 1 + dy][lx + 1 + dx], n1 = mag[ly + 1 - dy][lx + 1 - dx];
        const bool keep = m >= n0 && m >= n1;
        dst[(size_t)y * W + x] = (uint8_t)(keep ? (m >= hi ? 2 : (m >= lo ? 1 : 0)) : 0);
    }
}

// flags[0] = 1 (the carry-in of a group's first pass), flags[1 .. n] = 0
__global__ __launch_bounds__(64) void canny_flags_kernel(unsigned* flags, int n) {
    for (int i = threadIdx.x; i <= n; i += 64) flags[i] = i == 0 ? 1u : 0u;
}

__global__ __launch_bounds__(256) void canny_hysteresis_kernel(uint8_t* state, const unsigned* prev, unsigned* mine, int H, int W) {
    __shared__ uint8_t t[(kHH + 2) * kHS];
    __shared__ int flag[3];
    __shared__ int any_weak;
    if (*prev == 0u) return;                                             // the pass before changed nothing: fixed point reached
    const int b = blockIdx.z, x0 = blockIdx.x * kHW, y0 = blockIdx.y * kHH, tid = threadIdx.x;
    uint8_t* s = state + (size_t)b * H * W;
    if (tid == 0) { flag[0] = 0; flag[1] = 0; flag[2] = 0; any_weak = 0; }
    __syncthreads();
    int weak = 0;
    for (int i = tid; i < (kHH + 2) * (kHW + 2); i += 256) {
        const int ly = i / (kHW + 2), lx = i - ly * (kHW + 2);
        const int y = y0 + ly - 1, x = x0 + lx - 1;
        uint8_t v = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) v = s[(size_t)y * W + x];
        t[ly * kHS + lx] = v;
        weak |= (v == 1 && ly >= 1 && ly <= kHH && lx >= 1 && lx <= kHW);
    }
    if (weak) any_weak = 1;
    __syncthreads();
    if (!any_weak) return;                                               // uniform: nothing in this tile can change
    const int ry = tid >> 3, rx = (tid & 7) * 8;                         // this thread's run: row ry, columns rx .. rx + 7
    uint8_t* row = t + (ry + 1) * kHS + rx + 1;
    unsigned grown = 0;                                                  // bit e: pixel e of the run turned strong in this pass
    for (int it = 0;; ++it) {
        if (tid == 0) flag[(it + 1) % 3] = 0;
        int changed = 0;
        for (int sweep = 0; sweep < 2; ++sweep)                          // forward then backward: a chain along the run in one go
            for (int k = 0; k < 8; ++k) {
                const int e = sweep == 0 ? k : 7 - k;
                uint8_t* p = row + e;
                if (*p != 1) continue;
                if (p[-kHS - 1] == 2 || p[-kHS] == 2 || p[-kHS + 1] == 2 || p[-1] == 2 || p[1] == 2 || p[kHS - 1] == 2 ||
                    p[kHS] == 2 || p[kHS + 1] == 2) {
                    *p = 2;
                    grown |= 1u << e;
                    changed = 1;
                }
            }
        if (changed) flag[it % 3] = 1;
        __syncthreads();
        if (!flag[it % 3]) break;
    }
    if (grown) {
        const int y = y0 + ry;                                           // a grown pixel was weak in the image, so it lies inside it
        for (int e = 0; e < 8; ++e)
            if (grown & (1u << e)) s[(size_t)y * W + x0 + rx + e] = 2;
        atomicOr(mine, 1u);
    }
}

// V pixels per thread (V divides H*W, so a thread's pixels lie in one image)
template <int V>
__global__ __launch_bounds__(256) void canny_emit_kernel(const uint8_t* state, uint8_t* edges, half_t* guide, size_t HW, size_t total) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t base = i * V, b = base / HW, p = base - b * HW;
        uint8_t v[V];
        if (V == 8) {
            const uint64_t w = *reinterpret_cast<const uint64_t*>(state + base);
            __builtin_memcpy(v, &w, 8);
        } else {
            v[0] = state[base];
        }
        if (edges) {
            uint8_t o[V];
            for (int e = 0; e < V; ++e) o[e] = v[e] == 2 ? 255 : 0;
            if (V == 8) {
                uint64_t w;
                __builtin_memcpy(&w, o, 8);
                *reinterpret_cast<uint64_t*>(edges + base) = w;
            } else {
                edges[base] = o[0];
            }
        }
        if (guide) {
            for (int c = 0; c < 3; ++c) {
                half_t* g = guide + (b * 3 + c) * HW + p;
                if (V == 8) {
                    half8 o;
                    for (int e = 0; e < 8; ++e) o[e] = v[e] == 2 ? (half_t)1.0f : (half_t)-1.0f;
                    st8(g, o);
                } else {
                    g[0] = v[0] == 2 ? (half_t)1.0f : (half_t)-1.0f;
                }
            }
        }
    }
}

bool dims_ok(int B, int H, int W) {
    return B > 0 && H > 0 && W > 0 && B <= 65535 && (H + kCH - 1) / kCH <= 65535 && (long)B * H * W <= 0x7fffffffL;
}

}  // namespace

extern "C" int clora_canny_classify_u8(const uint8_t* img, const float* low, const float* high, uint8_t* cls, int B, int H, int W, int C,
                                       void* stream) {
    if (!img || !low || !high || !cls || !dims_ok(B, H, W) || (C != 1 && C != 3)) return CLORA_ERR_ARG;
    hipLaunchKernelGGL(canny_classify_kernel, dim3(clora_cdiv(W, kCW), clora_cdiv(H, kCH), B), dim3(256), 0, (hipStream_t)stream, img, low,
                       high, cls, H, W, C);
    return clora_check_launch();
}

extern "C" int clora_canny_hysteresis_u8(uint8_t* state, unsigned* flags, int pass_base, int npasses, int B, int H, int W, void* stream) {
    if (!state || !flags || !dims_ok(B, H, W) || npasses <= 0 || npasses > CLORA_CANNY_MAX_GROUP || pass_base < 0) return CLORA_ERR_ARG;
    if ((long)pass_base > (long)H * W) return CLORA_ERR_ARG;             // every pass but the last turns a weak pixel strong
    hipLaunchKernelGGL(canny_flags_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, flags, npasses);
    for (int i = 1; i <= npasses; ++i)
        hipLaunchKernelGGL(canny_hysteresis_kernel, dim3(clora_cdiv(W, kHW), clora_cdiv(H, kHH), B), dim3(256), 0, (hipStream_t)stream, state,
                           (const unsigned*)(flags + i - 1), flags + i, H, W);
    return clora_check_launch();
}

extern "C" int clora_canny_emit(const uint8_t* state, uint8_t* edges, clora_half* guide, int B, int H, int W, void* stream) {
    if (!state || (!edges && !guide) || !dims_ok(B, H, W)) return CLORA_ERR_ARG;
    const size_t HW = (size_t)H * W, n = (size_t)B * HW;
    const bool aligned = (((uintptr_t)state | (uintptr_t)edges) & 7) == 0 && ((uintptr_t)guide & 15) == 0;
    if (HW % 8 == 0 && aligned) {
        const size_t total = n / 8, blocks = (total + 255) / 256;
        hipLaunchKernelGGL(canny_emit_kernel<8>, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, (hipStream_t)stream, state, edges,
                           (half_t*)guide, HW, total);
    } else {
        const size_t blocks = (n + 255) / 256;
        hipLaunchKernelGGL(canny_emit_kernel<1>, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, (hipStream_t)stream, state, edges,
                           (half_t*)guide, HW, n);
    }
    return clora_check_launch();
}
