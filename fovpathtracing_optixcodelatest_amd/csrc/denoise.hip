// denoise.hip -- fovpt_denoise: a foveation-aware edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over the
// denoiser guides of a rendered frame (color = accum, normal, albedo; fovpt_config.write_guides = 1).
//
//   k_denoise_prep   level map (the pass of each pixel's last writer: its fill and iteration count), albedo
//                    demodulation I = C / D; pixels that are not filtered get their output here (C itself, bit for bit)
//   k_denoise_step   one a-trous iteration (5 x 5 taps at step fill * 2^i, B3-spline weights, colour / normal / albedo
//                    edge stopping) over the pixels with i < n; the last one remodulates and tone-maps into the outputs
//
// One thread per pixel, 64 x 4 pixel tiles (a wave reads 64 consecutive pixels of a tap row).  The definition, operation
// by operation, is tests/denoise_ref.py; -ffp-contract=off keeps every product and sum of it a separate binary32 op.
#include "fovpt_device.h"
#include "fovpt_pixel.h"

namespace {

// level byte: iterations n in bits 0-3, log2(fill) in bits 4-7 (fill 1, 2, 4)
__device__ inline V3 demod(const fovpt_float4& a)
{
    const float s = a.x + a.y + a.z;
    if (s > 0.0f) return v3(fmaxf(a.x, 1.0f / 64.0f), fmaxf(a.y, 1.0f / 64.0f), fmaxf(a.z, 1.0f / 64.0f));
    return v3(1.0f);
}
__device__ inline V3 div3(const V3& a, const V3& b) { return v3(a.x / b.x, a.y / b.y, a.z / b.z); }
__device__ inline float sq3(const V3& a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
__device__ inline float edge(float d) { const float t = fmaxf(0.0f, 1.0f - d); return t * t; }
__device__ inline bool is_zero(const V3& n) { return n.x == 0.0f && n.y == 0.0f && n.z == 0.0f; }
__device__ inline void write_out(fovpt_float4* out_color, uint32_t* out_rgba, uint32_t idx, const V3& c)
{
    out_color[idx] = fovpt_float4{c.x, c.y, c.z, 1.0f};
    out_rgba[idx] = make_color(reinhard(c * 16.0f, 1.0f));
}

__global__ __launch_bounds__(FOVPT_BLOCK) void k_denoise_prep(const FrameDev fd, DenoiseArgs a, const fovpt_float4* __restrict__ color,
                                                              const fovpt_float4* __restrict__ albedo, float4* __restrict__ I0,
                                                              uint8_t* __restrict__ level, fovpt_float4* __restrict__ out_color,
                                                              uint32_t* __restrict__ out_rgba)
{
    const uint32_t x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= (uint32_t)fd.w || y >= (uint32_t)fd.h) return;
    const uint32_t idx = y * (uint32_t)fd.w + x;
    int wp = 0, n = 0, sh = 0;
    uint32_t wlx, wly;
    if (find_last_writer(fd, x, y, wp, wlx, wly)) {
        n = a.n_pass[wp];
        sh = 31 - __clz(fd.pass[wp].fill);
    }
    level[idx] = (uint8_t)(n | (sh << 4));
    const fovpt_float4 c = color[idx];
    const V3 C = v3(c.x, c.y, c.z);
    const V3 I = div3(C, demod(albedo[idx]));
    I0[idx] = f4(I, 0.0f);
    if (n == 0) write_out(out_color, out_rgba, idx, C);
}

template <bool LAST>
__global__ __launch_bounds__(FOVPT_BLOCK) void k_denoise_step(int w, int h, int it, float kc, float inv_n, float inv_a,
                                                              const uint8_t* __restrict__ level, const float4* __restrict__ Iin,
                                                              const fovpt_float4* __restrict__ normal, const fovpt_float4* __restrict__ albedo,
                                                              float4* __restrict__ Iout, fovpt_float4* __restrict__ out_color,
                                                              uint32_t* __restrict__ out_rgba)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const uint32_t idx = (uint32_t)y * (uint32_t)w + (uint32_t)x;
    const int code = level[idx], n = code & 15;
    const V3 Ip = v3(Iin[idx]);
    if (it >= n) {                                       // done (or never filtered): keep I; the last launch remodulates
        if (!LAST) Iout[idx] = f4(Ip, 0.0f);
        else if (n >= 1) write_out(out_color, out_rgba, idx, Ip * demod(albedo[idx]));
        return;
    }
    const fovpt_float4 np4 = normal[idx], ap4 = albedo[idx];
    const V3 Np = v3(np4.x, np4.y, np4.z), Ap = v3(ap4.x, ap4.y, ap4.z);
    const bool np0 = is_zero(Np);
    const int s = 1 << ((code >> 4) + it);               // fill * 2^it: a block-filled pixel never taps its own copies
    const float lp = 0.2126f * Ip.x + 0.7152f * Ip.y + 0.0722f * Ip.z;
    const float k = kc / (1e-4f + lp * lp);
    const float H[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    float sw = 0.0f;
    V3 acc = v3(0.0f);
    // one tap row per trip (its 15 loads in flight together); unrolling all 25 taps needs 218 VGPRs (2 waves per SIMD)
#pragma unroll 1
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = min(max(y + s * dy, 0), h - 1);
        const float hy = dy == 0 ? 3.0f / 8.0f : (dy == 1 || dy == -1) ? 1.0f / 4.0f : 1.0f / 16.0f;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = min(max(x + s * dx, 0), w - 1);
            const uint32_t q = (uint32_t)qy * (uint32_t)w + (uint32_t)qx;
            const V3 Iq = v3(Iin[q]);
            const fovpt_float4 nq4 = normal[q], aq4 = albedo[q];
            const V3 Nq = v3(nq4.x, nq4.y, nq4.z), Aq = v3(aq4.x, aq4.y, aq4.z);
            const float wc = edge(sq3(Iq - Ip) * k);
            const bool nq0 = is_zero(Nq);
            const float wn = (np0 && nq0) ? 1.0f : (np0 || nq0) ? 0.0f : edge(sq3(Nq - Np) * inv_n);
            const float wa = edge(sq3(Aq - Ap) * inv_a);
            const float wt = ((H[dx + 2] * hy * wc) * wn) * wa;
            sw = sw + wt;
            acc = acc + Iq * wt;
        }
    }
    const V3 I = v3(acc.x / sw, acc.y / sw, acc.z / sw);   // sw >= 9/64: the centre tap
    if (!LAST) Iout[idx] = f4(I, 0.0f);
    else write_out(out_color, out_rgba, idx, I * demod(ap4));
}

}  // namespace

void fovpt_launch_denoise(hipStream_t st, const FrameDev& fd, const DenoiseArgs& a, const fovpt_float4* color, const fovpt_float4* normal,
                          const fovpt_float4* albedo, float4* I0, float4* I1, uint8_t* level, fovpt_float4* out_color, uint32_t* out_rgba)
{
    const dim3 grid((fd.w + 63) / 64, (fd.h + 3) / 4);
    hipLaunchKernelGGL(k_denoise_prep, grid, dim3(FOVPT_BLOCK), 0, st, fd, a, color, albedo, I0, level, out_color, out_rgba);
    float4* buf[2] = {I0, I1};
    for (int i = 0; i < a.iterations; i++) {
        const float kc = a.inv_c * (float)(1u << (2 * i));        // the colour scale shrinks by 2 per iteration (x 4 on d)
        if (i + 1 < a.iterations)
            hipLaunchKernelGGL(k_denoise_step<false>, grid, dim3(FOVPT_BLOCK), 0, st, fd.w, fd.h, i, kc, a.inv_n, a.inv_a, level, buf[i & 1],
                               normal, albedo, buf[(i + 1) & 1], out_color, out_rgba);
        else
            hipLaunchKernelGGL(k_denoise_step<true>, grid, dim3(FOVPT_BLOCK), 0, st, fd.w, fd.h, i, kc, a.inv_n, a.inv_a, level, buf[i & 1],
                               normal, albedo, buf[(i + 1) & 1], out_color, out_rgba);
    }
}
