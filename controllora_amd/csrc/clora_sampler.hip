// clora_sampler.hip -- one scheduler step of the sampling loop in ONE launch: the classifier-free-guidance combine of the UNet's
// two halves, the sampler update of the fp32 state (DDIM with any eta, DPM-Solver++ of first and second order: one linear form per
// element, the coefficients come from the host), and the next UNet input -- the fp16 copy of the new state in both halves of the CFG
// batch and the next timestep.  Between two UNet evaluations nothing else has to run.
//
// A thread owns ONE pixel with all of its C channels.  The state planes are channel-major (NCHW): for a fixed channel the lanes of
// a wave read 64 consecutive floats.  The noise prediction is read through four element strides: as a dense NCHW tensor (the same
// pattern, 2 bytes per lane), or as the view the UNet returns -- pixel-major rows of the padded conv_out width with the channels
// innermost -- where a pixel's 4 channels are one 8-byte load and consecutive lanes read consecutive rows.  Launch-bound at every
// latent size of the path (64 KB .. 1 MB per tensor), so there is no wider vector form.
#include "clora_common.h"
#include "../../include/clora.h"

namespace {

#define SAMPLER_MAX_BLOCKS 1024      // 4 blocks of 256 threads on each of the 256 CUs; more pixels than that take further trips

struct SamplerArgs {
    const half_t* eps;
    long long es_n, es_c, es_h, es_w;
    float* x;
    float* hist;
    const float* noise;
    half_t* x_in;
    long long* t_in;
    long long t_next;
    int B, C, H, W;
    clora_sampler_coef_t k;
};

// the three lines of include/clora.h, fp32 throughout; `h` and `nz` are only used where their coefficient is not zero
__device__ __forceinline__ void sampler_element(const clora_sampler_coef_t& k, float eu, float ec, float xv, float h, float nz, bool use_h,
                                                bool use_n, float& x0, float& xn) {
    const float e = eu + k.guidance * (ec - eu);
    x0 = k.x0_x * xv + k.x0_e * e;
    float acc = k.k_x * xv + k.k_x0 * x0;
    if (use_h) acc += k.k_h * h;
    acc += k.k_e * e;
    if (use_n) acc += k.k_n * nz;
    xn = acc;
}

// VEC4: C == 4 with the channels innermost (es_c == 1) and every pixel's four 8-byte aligned -- one load per pixel and half
template <bool VEC4>
__global__ __launch_bounds__(256) void sampler_step_kernel(SamplerArgs p) {
    const int C = VEC4 ? 4 : p.C;
    const size_t HW = (size_t)p.H * p.W;
    const size_t npix = (size_t)p.B * HW;
    const bool use_h = p.hist != nullptr && p.k.k_h != 0.f;
    const bool use_n = p.k.k_n != 0.f;
    if (p.t_in != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *p.t_in = p.t_next;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) {
        const size_t b = i / HW, hw = i - b * HW;
        const size_t h = hw / p.W, w = hw - h * p.W;
        const half_t* eu = p.eps + (long long)b * p.es_n + (long long)h * p.es_h + (long long)w * p.es_w;
        const half_t* ec = p.eps + (long long)(b + p.B) * p.es_n + (long long)h * p.es_h + (long long)w * p.es_w;
        const size_t plane = b * C * HW + hw;                        // channel 0 of this pixel in x / hist / noise / x_in's first half
        const size_t cond = (size_t)p.B * C * HW;                    // from a sample to its twin in x_in's second half
        half4v vu = {0, 0, 0, 0}, vc = {0, 0, 0, 0};
        if (VEC4) {
            vu = ld4(eu);
            vc = ld4(ec);
        }
#pragma unroll 4
        for (int c = 0; c < C; ++c) {
            const size_t at = plane + (size_t)c * HW;
            const float fu = VEC4 ? (float)vu[c & 3] : (float)eu[(long long)c * p.es_c];
            const float fc = VEC4 ? (float)vc[c & 3] : (float)ec[(long long)c * p.es_c];
            const float hv = use_h ? p.hist[at] : 0.f;
            const float nz = use_n ? p.noise[at] : 0.f;
            const float xv = p.x[at];
            float x0, xn;
            sampler_element(p.k, fu, fc, xv, hv, nz, use_h, use_n, x0, xn);
            p.x[at] = xn;
            if (p.hist != nullptr) p.hist[at] = x0;
            if (p.x_in != nullptr) {
                const half_t r = (half_t)xn;                          // round-to-nearest-even of the fp32 value just stored
                p.x_in[at] = r;
                p.x_in[at + cond] = r;
            }
        }
    }
}

}  // namespace

extern "C" int clora_sampler_step_f16(const clora_half* eps, long long es_n, long long es_c, long long es_h, long long es_w,
                                      float* x, float* hist, const float* noise, clora_half* x_in, long long* t_in,
                                      long long t_next, int B, int C, int H, int W, const clora_sampler_coef_t* coef, void* stream) {
    if (!eps || !x || !coef || B < 1 || C < 1 || H < 1 || W < 1) return CLORA_ERR_ARG;
    if (es_n == 0 || es_c == 0 || es_h == 0 || es_w == 0) return CLORA_ERR_ARG;
    if (coef->k_n != 0.f && !noise) return CLORA_ERR_ARG;
    SamplerArgs p;
    p.eps = (const half_t*)eps;
    p.es_n = es_n; p.es_c = es_c; p.es_h = es_h; p.es_w = es_w;
    p.x = x; p.hist = hist; p.noise = noise; p.x_in = (half_t*)x_in; p.t_in = t_in; p.t_next = t_next;
    p.B = B; p.C = C; p.H = H; p.W = W;
    const bool vec4 = C == 4 && es_c == 1 && ((uintptr_t)eps & 7) == 0 && (es_n & 3) == 0 && (es_h & 3) == 0 && (es_w & 3) == 0;
    p.k = *coef;
    const size_t npix = (size_t)B * H * W;
    const size_t blocks = (npix + 255) / 256;
    const dim3 grid((unsigned)(blocks > SAMPLER_MAX_BLOCKS ? SAMPLER_MAX_BLOCKS : blocks));
    if (vec4)
        hipLaunchKernelGGL(sampler_step_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(sampler_step_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, p);
    return clora_check_launch();
}
