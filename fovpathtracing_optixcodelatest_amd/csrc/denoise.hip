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
#include "fovpt_post_pixel.h"      // demod, edge, the a-trous level byte, weights and taps

namespace {

__device__ inline bool is_zero(const V3& n) { return n.x == 0.0f && n.y == 0.0f && n.z == 0.0f; }

__global__ __launch_bounds__(FOVPT_BLOCK) void k_denoise_prep(const FrameDev fd, DenoiseArgs a, const fovpt_float4* __restrict__ color,
                                                              const fovpt_float4* __restrict__ albedo, float4* __restrict__ I0,
                                                              uint8_t* __restrict__ level, fovpt_float4* __restrict__ out_color,
                                                              uint32_t* __restrict__ out_rgba)
{
    uint32_t x, y, idx;
    if (!tile_pixel(fd.w, fd.h, x, y, idx)) return;
    const AtrousLevel l = atrous_level(fd, a.n_pass, x, y);
    level[idx] = l.code();
    const V3 C = v3(color[idx]);
    const V3 I = div3(C, demod(v3(albedo[idx])));
    I0[idx] = f4(I, 0.0f);
    if (l.n == 0) store_resolved(out_color, out_rgba, idx, C);
}

template <bool LAST>
__global__ __launch_bounds__(FOVPT_BLOCK) void k_denoise_step(int w, int h, int it, float kc, float inv_n, float inv_a,
                                                              const uint8_t* __restrict__ level, const float4* __restrict__ Iin,
                                                              const fovpt_float4* __restrict__ normal, const fovpt_float4* __restrict__ albedo,
                                                              float4* __restrict__ Iout, fovpt_float4* __restrict__ out_color,
                                                              uint32_t* __restrict__ out_rgba)
{
    int x, y;
    uint32_t idx;
    if (!tile_pixel(w, h, x, y, idx)) return;
    const AtrousLevel l = atrous_decode(level[idx]);
    const V3 Ip = v3(Iin[idx]);
    if (it >= l.n) {                                       // done (or never filtered): keep I; the last launch remodulates
        if (!LAST) Iout[idx] = f4(Ip, 0.0f);
        else if (l.n >= 1) store_resolved(out_color, out_rgba, idx, Ip * demod(v3(albedo[idx])));
        return;
    }
    const V3 Np = v3(normal[idx]), Ap = v3(albedo[idx]);
    const bool np0 = is_zero(Np);
    const int s = 1 << (l.fill_shift + it);                       // fill * 2^it: a block-filled pixel never taps its own copies
    const float lp = luma(Ip);
    const float k = kc / (1e-4f + lp * lp);
    float sw = 0.0f;
    V3 acc = v3(0.0f);
    // one tap row per trip (its 15 loads in flight together); unrolling all 25 taps needs 218 VGPRs (2 waves per SIMD)
#pragma unroll 1
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = tap_coord(y, s, dy, h);
        const float hy = b3_weight_row(dy);
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const uint32_t q = (uint32_t)qy * (uint32_t)w + (uint32_t)tap_coord(x, s, dx, w);
            const V3 Iq = v3(Iin[q]), Nq = v3(normal[q]), Aq = v3(albedo[q]);
            const float wc = edge(sq3(Iq - Ip) * k);
            const bool nq0 = is_zero(Nq);
            const float wn = (np0 && nq0) ? 1.0f : (np0 || nq0) ? 0.0f : edge(sq3(Nq - Np) * inv_n);
            const float wa = edge(sq3(Aq - Ap) * inv_a);
            const float wt = ((b3_weight(dx) * hy * wc) * wn) * wa;
            sw = sw + wt;
            acc = acc + Iq * wt;
        }
    }
    const V3 I = div3(acc, sw);                          // sw >= 9/64: the centre tap
    if (!LAST) Iout[idx] = f4(I, 0.0f);
    else store_resolved(out_color, out_rgba, idx, I * demod(Ap));
}

}  // namespace

void fovpt_launch_denoise(hipStream_t st, const FrameDev& fd, const DenoiseArgs& a, const fovpt_float4* color, const fovpt_float4* normal,
                          const fovpt_float4* albedo, float4* I0, float4* I1, uint8_t* level, fovpt_float4* out_color, uint32_t* out_rgba)
{
    const dim3 grid = fovpt_tile_grid(fd.w, fd.h);
    hipLaunchKernelGGL(k_denoise_prep, grid, dim3(FOVPT_BLOCK), 0, st, fd, a, color, albedo, I0, level, out_color, out_rgba);
    fovpt_atrous_iterate(a.iterations, I0, I1, [&](int i, bool last, const float4* Iin, float4* Iout) {
        const float kc = a.inv_c * (float)(1u << (2 * i));        // the colour scale shrinks by 2 per iteration (x 4 on d)
        hipLaunchKernelGGL(!last ? k_denoise_step<false> : k_denoise_step<true>, grid, dim3(FOVPT_BLOCK), 0, st, fd.w, fd.h, i, kc, a.inv_n,
                           a.inv_a, level, Iin, normal, albedo, Iout, out_color, out_rgba);
    });
}
