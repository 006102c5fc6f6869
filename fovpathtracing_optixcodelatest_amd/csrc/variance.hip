// variance.hip -- fovpt_variance and fovpt_variance_filter: temporally reprojected luminance moments with a spatial fallback, and an
// a-trous filter whose luminance edge-stop is scaled by the variance they give (after Schied et al. 2017, SVGF), over a per-pixel
// G-buffer of the rendered frame (fovpt_gbuffer's or a temporal step's), not over the frame's guides.
//
//   k_variance_moments  per pixel: luminance and its square, the four bilinear taps of the previous moment history where the motion
//                       vector lands (kept by class and depth), the blend by history length, the variance -- from the moments, or
//                       from a (2R + 1)^2 window of the current frame while the history is short -- and the new history record
//   k_vfilter_prep      level map (atrous_level, fovpt_post_pixel.h), demodulation by the G-buffer's albedo, J = (I, rel * lum(I)^2); pixels that are
//                       not filtered get their output here (C itself, bit for bit)
//   k_vfilter_step      one iteration over the pixels with i < n: the 3 x 3 prefilter of the variance, 5 x 5 taps at step fill * 2^i
//                       with B3-spline weights and luminance / normal / plane-distance edge stopping, the filtered variance; the
//                       last one remodulates and tone-maps into the outputs
//
// One thread per pixel, 64 x 4 pixel tiles, one tap row per loop trip (as k_denoise_step).  The definition, operation by operation,
// is tests/variance_ref.py; -ffp-contract=off keeps every product and sum of it a separate binary32 op.
#include "fovpt_device.h"
#include "fovpt_pixel.h"
#include "fovpt_post_pixel.h"      // demod, edge, sq3, the a-trous level byte, weights and taps

namespace {

// The spatial estimate's sums over the (2R + 1)^2 window of pixel (x, y), stepping by the fill f: one tap row per trip, its loads in
// flight together (R is a template argument so that the row unrolls)
struct Window { int w, h, x, y, f; bool miss_p; V3 Xp, Np; float ztol, ntol; };
template <int R>
__device__ inline void window(const Window& d, const fovpt_float4* __restrict__ in, const float4* __restrict__ pos, const float4* __restrict__ nrm,
                              float& s0, float& s1, float& s2)
{
#pragma unroll 1
    for (int j = -R; j <= R; j++) {
        const int qy = tap_coord(d.y, d.f, j, d.h);
#pragma unroll
        for (int i = -R; i <= R; i++) {
            const uint32_t q = (uint32_t)qy * (uint32_t)d.w + (uint32_t)tap_coord(d.x, d.f, i, d.w);
            const fovpt_float4 cq = in[q];
            const float4 xq4 = pos[q];
            float wq = 1.0f;
            if (i != 0 || j != 0) {
                if ((xq4.w < 0.0f) != d.miss_p) wq = 0.0f;
                else if (!d.miss_p) {
                    const V3 Nq = v3(nrm[q]);
                    if (!(sq3(Nq - d.Np) <= d.ntol) || !(fabsf(dot(d.Np, v3(xq4) - d.Xp)) <= d.ztol)) wq = 0.0f;
                }
            }
            const float lq = luma(v3(cq));
            s0 = s0 + wq;
            s1 = s1 + wq * lq;
            s2 = s2 + wq * (lq * lq);
        }
    }
}

__global__ __launch_bounds__(FOVPT_BLOCK) void k_variance_moments(const FrameDev fd, const VarianceArgs a, const fovpt_float4* __restrict__ in,
                                                                  const float4* __restrict__ pos, const float4* __restrict__ nrm,
                                                                  const fovpt_float4* __restrict__ motion, const float4* __restrict__ hist_prev,
                                                                  float4* __restrict__ hist_out, fovpt_float4* __restrict__ out)
{
    const int w = fd.w, h = fd.h;
    int x, y;
    uint32_t idx;
    if (!tile_pixel(w, h, x, y, idx)) return;
    const float l = luma(v3(in[idx])), l2 = l * l;
    const float4 xp4 = pos[idx];
    const bool miss_p = xp4.w < 0.0f;
    const V3 Xp = v3(xp4);
    float zp = -1.0f;
    if (!miss_p) {
        const V3 v = Xp - v3(a.eye[0], a.eye[1], a.eye[2]);
        zp = (a.m2[0] * v.x + a.m2[1] * v.y) + a.m2[2] * v.z;
    }
    // the history where the pixel was
    float m1 = 0.0f, m2 = 0.0f, nh = 0.0f;
    if (a.has_history) {
        float mx = 0.0f, my = 0.0f, zr = zp, mw = 1.0f;
        if (motion) { const fovpt_float4 mv = motion[idx]; mx = mv.x; my = mv.y; zr = mv.z; mw = mv.w; }
        const float px = (float)x + mx, py = (float)y + my;
        if (!(mw == 0.0f) && px >= -1.0f && px < (float)w && py >= -1.0f && py < (float)h) {   // (NaN fails): x0 in [-1, w - 1], y0 in [-1, h - 1]
            const float x0f = floorf(px), y0f = floorf(py);
            const float fx = px - x0f, fy = py - y0f;
            const int x0 = (int)x0f, y0 = (int)y0f;
            const float wt[4] = {(1.0f - fx) * (1.0f - fy), fx * (1.0f - fy), (1.0f - fx) * fy, fx * fy};
            const float ztol = a.depth_tol * zr;
            float sw = 0.0f, s1 = 0.0f, s2 = 0.0f, sn = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
                if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                const float4 hq = hist_prev[(uint32_t)qy * (uint32_t)w + (uint32_t)qx];
                if ((hq.w < 0.0f) != miss_p) continue;
                if (!miss_p && !(fabsf(hq.w - zr) <= ztol)) continue;
                sw = sw + wt[k];
                s1 = s1 + hq.x * wt[k];
                s2 = s2 + hq.y * wt[k];
                sn = sn + hq.z * wt[k];
            }
            if (sw >= 1.0f / 64.0f) { m1 = s1 / sw; m2 = s2 / sw; nh = sn / sw; }
        }
    }
    const float n = fminf(nh + 1.0f, (float)a.cap);
    float M1 = l, M2 = l2;
    if (n != 1.0f) {
        const float t = 1.0f / n;
        M1 = m1 + t * (l - m1);
        M2 = m2 + t * (l2 - m2);
    }
    hist_out[idx] = make_float4(M1, M2, n, zp);
    float mean = M1, var = fmaxf(0.0f, M2 - M1 * M1);
    if (!(n >= (float)a.spatial_below)) {                                  // a short history: the window of the current frame
        int f = 1, wp = 0;
        uint32_t wlx, wly;
        if (find_last_writer(fd, (uint32_t)x, (uint32_t)y, wp, wlx, wly)) f = fd.pass[wp].fill;
        const V3 Np = v3(nrm[idx]);
        const float ztol = a.depth_tol * xp4.w;
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
        const Window wd = {w, h, x, y, f, miss_p, Xp, Np, ztol, a.normal_tol};
        if (a.radius == 1) window<1>(wd, in, pos, nrm, s0, s1, s2);
        else if (a.radius == 2) window<2>(wd, in, pos, nrm, s0, s1, s2);
        else window<3>(wd, in, pos, nrm, s0, s1, s2);
        mean = s1 / s0;
        var = fmaxf(0.0f, s2 / s0 - mean * mean);
    }
    out[idx] = fovpt_float4{var / (mean * mean + 1e-8f), var, mean, n};
}

__global__ __launch_bounds__(FOVPT_BLOCK) void k_vfilter_prep(const FrameDev fd, VFilterArgs a, const fovpt_float4* __restrict__ color,
                                                              const fovpt_float4* __restrict__ variance, const float4* __restrict__ albedo,
                                                              float4* __restrict__ J0, uint8_t* __restrict__ level, fovpt_float4* __restrict__ out_color,
                                                              uint32_t* __restrict__ out_rgba)
{
    uint32_t x, y, idx;
    if (!tile_pixel(fd.w, fd.h, x, y, idx)) return;
    const AtrousLevel l = atrous_level(fd, a.n_pass, x, y);
    level[idx] = l.code();
    const V3 C = v3(color[idx]);
    const V3 D = a.demodulate ? demod(v3(albedo[idx])) : v3(1.0f);
    const V3 I = v3(C.x / D.x, C.y / D.y, C.z / D.z);                      // (not div3: with this D it orders the kernel's code differently)
    const float lI = luma(I);
    J0[idx] = f4(I, variance[idx].x * (lI * lI));
    if (l.n == 0) store_resolved(out_color, out_rgba, idx, C);
}

template <bool LAST>
__global__ __launch_bounds__(FOVPT_BLOCK) void k_vfilter_step(int w, int h, int it, int demodulate, float sl2, float inv_n, float inv_z,
                                                              const uint8_t* __restrict__ level, const float4* __restrict__ Jin,
                                                              const float4* __restrict__ pos, const float4* __restrict__ nrm,
                                                              const float4* __restrict__ albedo, float4* __restrict__ Jout,
                                                              fovpt_float4* __restrict__ out_color, uint32_t* __restrict__ out_rgba)
{
    int x, y;
    uint32_t idx;
    if (!tile_pixel(w, h, x, y, idx)) return;
    const AtrousLevel l = atrous_decode(level[idx]);
    const float4 Jp = Jin[idx];
    const V3 Ip = v3(Jp);
    if (it >= l.n) {                                     // done (or never filtered): keep J; the last launch remodulates
        if (!LAST) Jout[idx] = Jp;
        else if (l.n >= 1) store_resolved(out_color, out_rgba, idx, demodulate ? Ip * demod(v3(albedo[idx])) : Ip);
        return;
    }
    const int f = 1 << l.fill_shift;
    const int s = f << it;                               // fill * 2^it: a block-filled pixel never taps its own copies
    // the variance, prefiltered over the 3 x 3 neighbours one fill away
    float g = 0.0f;
#pragma unroll
    for (int j = -1; j <= 1; j++) {
        const int qy = tap_coord(y, f, j, h);
#pragma unroll
        for (int i = -1; i <= 1; i++) {
            const int qx = tap_coord(x, f, i, w);
            const float G = (i == 0 ? 0.5f : 0.25f) * (j == 0 ? 0.5f : 0.25f);       // 1/4, 1/8, 1/16: exact
            g = g + G * Jin[(uint32_t)qy * (uint32_t)w + (uint32_t)qx].w;
        }
    }
    const float kl = 1.0f / (sl2 * g + 1e-6f);
    const float4 xp4 = pos[idx];
    const bool miss_p = xp4.w < 0.0f;
    const V3 Xp = v3(xp4), Np = v3(nrm[idx]);
    const float tp2 = xp4.w * xp4.w;
    const float lp = luma(Ip);
    float sw = 0.0f, sv = 0.0f;
    V3 acc = v3(0.0f);
    // one tap row per trip (its 15 loads in flight together), as k_denoise_step
#pragma unroll 1
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = tap_coord(y, s, dy, h);
        const float hy = b3_weight_row(dy);
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const uint32_t q = (uint32_t)qy * (uint32_t)w + (uint32_t)tap_coord(x, s, dx, w);
            const float4 Jq = Jin[q], xq4 = pos[q], nq4 = nrm[q];
            const V3 Iq = v3(Jq);
            const float d = luma(Iq) - lp;
            const float wl = edge((d * d) * kl);
            const bool miss_q = xq4.w < 0.0f;
            float wn = 1.0f, wz = 1.0f;
            if (miss_p != miss_q) wn = wz = 0.0f;
            else if (!miss_p) {
                wn = edge(sq3(v3(nq4) - Np) * inv_n);
                const float dz = dot(Np, v3(xq4) - Xp);
                wz = edge(((dz * dz) * inv_z) / tp2);
            }
            const float wt = (((b3_weight(dx) * hy) * wl) * wn) * wz;
            sw = sw + wt;
            acc = acc + Iq * wt;
            sv = sv + (wt * wt) * Jq.w;
        }
    }
    const V3 I = div3(acc, sw);                          // sw >= 9/64: the centre tap
    if (!LAST) Jout[idx] = f4(I, sv / (sw * sw));
    else store_resolved(out_color, out_rgba, idx, demodulate ? I * demod(v3(albedo[idx])) : I);
}

}  // namespace

void fovpt_launch_variance(hipStream_t st, const FrameDev& fd, const VarianceArgs& a, const fovpt_float4* in, const float4* pos, const float4* nrm,
                           const fovpt_float4* motion, const float4* hist_prev, float4* hist_out, fovpt_float4* out_variance)
{
    hipLaunchKernelGGL(k_variance_moments, fovpt_tile_grid(fd.w, fd.h), dim3(FOVPT_BLOCK), 0, st, fd, a, in, pos, nrm, motion, hist_prev,
                       hist_out, out_variance);
}

void fovpt_launch_vfilter(hipStream_t st, const FrameDev& fd, const VFilterArgs& a, const fovpt_float4* color, const fovpt_float4* variance,
                          GBufferDev g, float4* J0, float4* J1, uint8_t* level, fovpt_float4* out_color, uint32_t* out_rgba)
{
    const dim3 grid = fovpt_tile_grid(fd.w, fd.h);
    hipLaunchKernelGGL(k_vfilter_prep, grid, dim3(FOVPT_BLOCK), 0, st, fd, a, color, variance, g.alb, J0, level, out_color, out_rgba);
    fovpt_atrous_iterate(a.iterations, J0, J1, [&](int i, bool last, const float4* Jin, float4* Jout) {
        hipLaunchKernelGGL(!last ? k_vfilter_step<false> : k_vfilter_step<true>, grid, dim3(FOVPT_BLOCK), 0, st, fd.w, fd.h, i, a.demodulate, a.sl2,
                           a.inv_n, a.inv_z, level, Jin, g.pos, g.nrm, g.alb, Jout, out_color, out_rgba);
    });
}
