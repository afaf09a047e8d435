// clora_attn_common.h -- what the attention translation units share (clora_attn.hip: head dims <= 160, forward and backward;
// clora_attn_wide.hip: forward, head dims 161 .. 512): the launch arguments, the block -> (head, block) remap, the fragment reads and
// the LDS-DMA tile copy.  The register-level design they serve is described at the top of clora_attn.hip.
#pragma once
#include "clora_common.h"

struct AttnArgs {
    const half_t *q, *k, *v, *o, *dO;
    half_t *out, *dq, *dk, *dv;
    const float* lse_in;
    float *lse, *delta;
    int ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
    int B, H, Nq, Nk, D;
    float scale;
    int nsplit, q_per_split;   // dK/dV: split the query loop over grid.z (cross-attention: few keys, many queries)
    float* acc32;              // [2][B, Nk, H*D] fp32 accumulators for the split path
    int xcd_heads;             // block order: whole (batch, head) pairs per XCD (see attn_block_ids)
};

// forward for head dims 160 < D <= 512 (clora_attn_wide.hip); clora_attn_fwd_f16 validates the arguments and dispatches here
__attribute__((visibility("hidden"))) int clora_attn_fwd_wide(const AttnArgs& a, hipStream_t s);

namespace {

// The blocks of one (batch, head) read the same K / V (forward, dQ) or Q / dO (dK/dV) stream.  Workgroup L runs on XCD L % 8
// and a line is fetched through the fabric once per XCD that asks for it (tools/probes/l2_share_probe.hip): in launch order
// the blocks of a head sit on all eight XCDs.  With xcd_heads every XCD walks a contiguous range of (head, block) pairs, so
// a head's stream is fetched by one XCD (two at a range boundary).  Same remap as the GEMM tile order; results do not change.
__device__ __forceinline__ void attn_block_ids(const AttnArgs& p, int& bx, int& by) {
    bx = blockIdx.x; by = blockIdx.y;
    if (!p.xcd_heads || gridDim.z != 1) return;
    const int nx = gridDim.x, nwg = nx * gridDim.y;
    const int lin = by * nx + bx;
    const int xq = nwg >> 3, xr = nwg & 7, xcd = lin & 7;
    const int logical = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (lin >> 3);
    by = logical / nx;
    bx = logical - by * nx;
}

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
constexpr float kNegBig = -1.0e30f;

// A operand (k-slots = rows {pair*32 + 4g .. +3} and {pair*32 + 16 + 4g .. +3}, operand row = column col0 + li) straight
// from a ROW-MAJOR tile [row][col] with the gfx950 transpose read: the 16 lanes of group g
// address the 4 rows {pair*32 + 4g .. +3} x 16 columns {col0 ..} (4 lanes per row, 4 columns each) and lane li receives
// column col0 + li of those 4 rows; a second read 16 rows further down gives the other 4 k-slots.  The tile is written
// with 16-byte stores (no transposed 2-byte scatter) and needs no second, transposed copy in LDS.
template <int LD>
__device__ __forceinline__ half8 frag_tr(const half_t* tile, int col0, int pair, int g, int l) {
    const half_t* q = tile + (pair * 32 + 4 * g + ((l & 15) >> 2)) * LD + col0 + (l & 3) * 4;
    const half4v a = CLORA_DS_READ_TR16(q), b = CLORA_DS_READ_TR16(q + 16 * LD);
    half8 r;
    r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; r[3] = a[3];
    r[4] = b[0]; r[5] = b[1]; r[6] = b[2]; r[7] = b[3];
    return r;
}
// B operand from two C-layout tiles (same slot assignment as frag_tr)
__device__ __forceinline__ half8 frag_from_acc(floatx4 lo, floatx4 hi) {
    half8 r;
    r[0] = (half_t)lo[0]; r[1] = (half_t)lo[1]; r[2] = (half_t)lo[2]; r[3] = (half_t)lo[3];
    r[4] = (half_t)hi[0]; r[5] = (half_t)hi[1]; r[6] = (half_t)hi[2]; r[7] = (half_t)hi[3];
    return r;
}

// K / V / Q / dO tiles go global -> LDS by LDS-DMA (`global_load_lds_dwordx4`: no staging registers, no ds_write pass) into a
// DOUBLE-BUFFERED tile pair: the copy of tile t+1 is issued before the MFMAs of tile t and only has to have landed at the
// single barrier that ends the iteration (s_waitcnt vmcnt(0) + s_barrier) -- one barrier per tile instead of two, no exposed
// LDS write phase, and 16-32 VGPRs of staging registers returned to the loop.
// A tile is ROWS x (LD/8) 16-byte chunks, row pitch LD halves (the conflict-free padded pitch of the fragment reads); the
// DMA image is lane-linear, so one wave-instruction fills 64 consecutive chunk slots; the lane that owns slot s fetches
// chunk s % (LD/8) of row s / (LD/8) -- or a 16-byte zero page for the head-dim / row padding, or (ONE) the "one page"
// for the chunk that starts at column D: the ones column of V that makes P.V accumulate rowsum(P) (attn_fwd_kernel).
__device__ __attribute__((aligned(16))) const unsigned g_attn_zero16[4] = {0u, 0u, 0u, 0u};
__device__ __attribute__((aligned(16))) const unsigned short g_attn_one16[8] = {0x3C00u, 0, 0, 0, 0, 0, 0, 0};

template <int ROWS, int LD, int NWV = 4>
struct TileDma {
    static constexpr int PCH = LD / 8;                 // chunks per padded row
    static constexpr int NI = ROWS * PCH / 64;         // wave-instructions per tile
    static constexpr int NIW = (NI + NWV - 1) / NWV;   // ... per wave (wave w of NWV issues instructions w, w+NWV, ...)
    static_assert((ROWS * PCH) % 64 == 0, "a tile must be a whole number of DMA wave-instructions");
    int row[NIW], col[NIW];                            // this lane's (row, first column) per instruction; col -1: padding, -2: ones chunk
    __device__ __forceinline__ void init(int w, int l, int D) {
#pragma unroll
        for (int j = 0; j < NIW; ++j) {
            const int sl = (w + NWV * j) * 64 + l;
            const int r = sl / PCH, c = sl - r * PCH;
            row[j] = r;
            col[j] = (c * 8 < D) ? c * 8 : (c * 8 == D ? -2 : -1);
        }
    }
    template <bool ONE>
    __device__ __forceinline__ void issue(const half_t* base, int ld, int rows_valid, half_t* dst, int w) const {
        const half_t* zero_page = reinterpret_cast<const half_t*>(g_attn_zero16);
        const half_t* one_page = reinterpret_cast<const half_t*>(g_attn_one16);
#pragma unroll
        for (int j = 0; j < NIW; ++j) {
            const int i = w + NWV * j;
            if (i < NI) {
                const bool in = row[j] < rows_valid;       // selects, not branches: the issue path stays straight-line
                const half_t* src = (in && col[j] >= 0) ? base + row[j] * ld + col[j] : zero_page;
                if (ONE) src = (in && col[j] == -2) ? one_page : src;
                CLORA_GLDS16(src, dst + i * 512);
            }
        }
    }
};
__device__ __forceinline__ floatx4 splat4f(float x) {
    floatx4 z = {x, x, x, x};
    return z;
}
// the lazy exponent reference of the forward kernels follows the running maximum only when a tile exceeds it by more than 2^kRebase
constexpr float kRebase = 8.0f;

}  // namespace
