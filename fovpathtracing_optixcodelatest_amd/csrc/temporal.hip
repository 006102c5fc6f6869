// temporal.hip -- fovpt_temporal: the reprojection of a context's frame history onto the frame last rendered, with a history
// length capped per foveation level (cf. Nehab et al. 2007, Yang et al. 2009; no neighbourhood clamp: DESIGN.md, section 12).
//
//   k_temporal   per pixel: its G-buffer point (a hit) or its camera-ray direction (a miss) projected into the previous step's
//                camera, the four bilinear taps of the previous history kept where the previous G-buffer agrees (same class,
//                normal and plane distance within tolerance), then out = lerp(history, in, 1 / n) with n = min(n_h + 1, cap)
//
//   k_temporal_motion   fovpt_temporal_motion: k_temporal in which a hit pixel of a mesh that fovpt_update_vertices has moved
//                since the previous step takes its point and normal from its triangle's previous vertices, and which can
//                store per-pixel motion vectors (tests/temporal_motion_ref.py)
//
// One thread per pixel, 64 x 4 pixel tiles, no LDS.  The definition, operation by operation, is tests/temporal_ref.py;
// -ffp-contract=off keeps every product and sum of it a separate binary32 op.
#include "fovpt_device.h"
#include "fovpt_pixel.h"

namespace {

__device__ inline float sq3(const V3& a) { return a.x * a.x + a.y * a.y + a.z * a.z; }

// `in` and `out_color` may be the same buffer: a thread reads only its own pixel of `in`, before it writes out_color
__global__ __launch_bounds__(FOVPT_BLOCK) void k_temporal(const FrameDev fd, TemporalArgs a, const fovpt_float4* in, GBufferDev g, GBufferDev gp,
                                                          const float4* __restrict__ hist_prev, float4* __restrict__ hist_out,
                                                          fovpt_float4* out_color, uint32_t* __restrict__ out_rgba)
{
    const uint32_t x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= (uint32_t)fd.w || y >= (uint32_t)fd.h) return;
    const uint32_t idx = y * (uint32_t)fd.w + x;
    const fovpt_float4 c = in[idx];
    int cap = 1;
    int wp = 0;
    uint32_t wlx, wly;
    if (find_last_writer(fd, x, y, wp, wlx, wly)) {
        const int f = fd.pass[wp].fill;
        cap = a.uniform ? a.cap[3] : f == 4 ? a.cap[2] : f == 2 ? a.cap[1] : a.cap[0];
    }
    float nh = 0.0f;
    V3 H = v3(0.0f);
    if (a.reproject && cap > 1) {                                          // (cap 1: n is 1 whatever the history says)
        const bool miss_p = g.prim[idx] == 0xffffffffu;
        const float4 xp4 = g.pos[idx];
        const V3 Xp = v3(xp4);
        V3 v;
        if (!miss_p) v = Xp - v3(a.eye_prev[0], a.eye_prev[1], a.eye_prev[2]);
        else {                                                             // k_gbuffer_rays' direction, before normalising
            const float dx = 2.0f * (((float)x + 0.5f) / (float)fd.w) - 1.0f;
            const float dy = 2.0f * (((float)y + 0.5f) / (float)fd.h) - 1.0f;
            const V3 U = v3(fd.U[0], fd.U[1], fd.U[2]), V = v3(fd.V[0], fd.V[1], fd.V[2]), W = v3(fd.W[0], fd.W[1], fd.W[2]);
            v = dx * U + dy * V + W;
        }
        const float ax = (a.inv[0] * v.x + a.inv[1] * v.y) + a.inv[2] * v.z;
        const float ay = (a.inv[3] * v.x + a.inv[4] * v.y) + a.inv[5] * v.z;
        const float az = (a.inv[6] * v.x + a.inv[7] * v.y) + a.inv[8] * v.z;
        if (az > 0.0f) {
            const float fw = (float)fd.w, fh = (float)fd.h;
            const float px = (((ax / az) + 1.0f) * 0.5f) * fw - 0.5f;
            const float py = (((ay / az) + 1.0f) * 0.5f) * fh - 0.5f;
            if (px >= -1.0f && px < fw && py >= -1.0f && py < fh) {        // (NaN fails): x0 in [-1, w - 1], y0 in [-1, h - 1]
                const float x0f = floorf(px), y0f = floorf(py);
                const float fx = px - x0f, fy = py - y0f;
                const int x0 = (int)x0f, y0 = (int)y0f;
                const float wt[4] = {(1.0f - fx) * (1.0f - fy), fx * (1.0f - fy), (1.0f - fx) * fy, fx * fy};
                const V3 Np = v3(g.nrm[idx]);
                const float ztol = a.depth_tol * xp4.w;
                float sw = 0.0f, sn = 0.0f;
                V3 acc = v3(0.0f);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
                    if (qx < 0 || qx >= fd.w || qy < 0 || qy >= fd.h) continue;
                    const uint32_t q = (uint32_t)qy * (uint32_t)fd.w + (uint32_t)qx;
                    if ((gp.prim[q] == 0xffffffffu) != miss_p) continue;
                    if (!miss_p) {
                        const V3 Nq = v3(gp.nrm[q]), Xq = v3(gp.pos[q]);
                        if (!(sq3(Nq - Np) <= a.normal_tol)) continue;
                        if (!(fabsf(dot(Np, Xq - Xp)) <= ztol)) continue;
                    }
                    const float4 hq = hist_prev[q];
                    sw = sw + wt[k];
                    acc = acc + v3(hq) * wt[k];
                    sn = sn + hq.w * wt[k];
                }
                if (sw >= 1.0f / 64.0f) {
                    H = v3(acc.x / sw, acc.y / sw, acc.z / sw);
                    nh = sn / sw;
                }
            }
        }
    }
    const float n = fminf(nh + 1.0f, (float)cap);
    if (n == 1.0f) {                                                       // first step, disocclusion, cap 1: the input, bit for bit
        out_color[idx] = c;
        hist_out[idx] = make_float4(c.x, c.y, c.z, 1.0f);
        out_rgba[idx] = make_color(reinhard(v3(c.x, c.y, c.z) * 16.0f, 1.0f));
        return;
    }
    const V3 o = lerp3(H, v3(c.x, c.y, c.z), 1.0f / n);
    out_color[idx] = fovpt_float4{o.x, o.y, o.z, 1.0f};
    hist_out[idx] = f4(o, n);
    out_rgba[idx] = make_color(reinhard(o * 16.0f, 1.0f));
}

// k_temporal with a moving surface's point and normal taken where the surface was at the previous step (tests/temporal_motion_ref.py):
// a hit pixel whose mesh is marked (m.mark[mesh] == m.epoch) gets X' = (w0 a' + u b') + v c' and N' = normalize(cross(b' - a',
// c' - a')) * s from its triangle's previous vertices a', b', c' and its hit's (u, v), s the sign k_gbuffer_fill gave the current
// normal; every other pixel takes k_temporal's path with k_temporal's operations.  The common case -- an unmarked mesh -- pays
// for the hit record's last word, one word of the triangle record and the mark, not for the vertex gathers.  With m.out_motion the
// projection also runs for cap-1 pixels and (px - x, py - y, a.z, 1) is stored, (0, 0, 0, 0) where the pixel does not reproject.
__global__ __launch_bounds__(FOVPT_BLOCK) void k_temporal_motion(const FrameDev fd, TemporalArgs a, TemporalMotionArgs m, const fovpt_float4* in,
                                                                 GBufferDev g, GBufferDev gp, const float4* __restrict__ hist_prev,
                                                                 float4* __restrict__ hist_out, fovpt_float4* out_color,
                                                                 uint32_t* __restrict__ out_rgba)
{
    const uint32_t x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= (uint32_t)fd.w || y >= (uint32_t)fd.h) return;
    const uint32_t idx = y * (uint32_t)fd.w + x;
    const fovpt_float4 c = in[idx];
    int cap = 1;
    int wp = 0;
    uint32_t wlx, wly;
    if (find_last_writer(fd, x, y, wp, wlx, wly)) {
        const int f = fd.pass[wp].fill;
        cap = a.uniform ? a.cap[3] : f == 4 ? a.cap[2] : f == 2 ? a.cap[1] : a.cap[0];
    }
    const bool want_motion = m.out_motion != nullptr;                      // (wave-uniform: a kernel argument)
    float nh = 0.0f;
    V3 H = v3(0.0f);
    float4 mv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (a.reproject && (cap > 1 || want_motion)) {
        const uint32_t prim = g.prim[idx];
        const bool miss_p = prim == 0xffffffffu;
        const float4 xp4 = g.pos[idx];
        V3 Xp = v3(xp4), Np = v3(0.0f);
        V3 v;
        if (!miss_p) {
            Np = v3(g.nrm[idx]);
            const uint32_t rec = __float_as_uint(m.hit[idx].w) << 4;       // byte offset of the triangle record, as k_gbuffer_fill's
            const float4* tr = (const float4*)((const char*)m.tris + rec);
            const uint32_t mesh = __float_as_uint(tr[2].z);
            if (m.mark[mesh] == m.epoch) {
                const float4 hit = m.hit[idx];
                const uint3 iv = m.tri_vidx[prim];
                const float* pa = m.vtx_prev + 3 * (size_t)iv.x, *pb = m.vtx_prev + 3 * (size_t)iv.y, *pc = m.vtx_prev + 3 * (size_t)iv.z;
                const V3 A = v3(pa[0], pa[1], pa[2]), B = v3(pb[0], pb[1], pb[2]), Cc = v3(pc[0], pc[1], pc[2]);
                const float w0 = (1.0f - hit.y) - hit.z;
                Xp = (w0 * A + hit.y * B) + hit.z * Cc;
                // s: k_gbuffer_fill's copysignf(1, dot(wo, N_0)) over the current record's edges and k_gbuffer_rays' direction
                const float4 t0 = tr[0], t1 = tr[1];
                const V3 N_0 = normalize(cross(v3(t0.w, t1.x, t1.y), v3(t1.z, t1.w, tr[2].x)));
                const float dx = 2.0f * (((float)x + 0.5f) / (float)fd.w) - 1.0f;
                const float dy = 2.0f * (((float)y + 0.5f) / (float)fd.h) - 1.0f;
                const V3 U = v3(fd.U[0], fd.U[1], fd.U[2]), V = v3(fd.V[0], fd.V[1], fd.V[2]), W = v3(fd.W[0], fd.W[1], fd.W[2]);
                const V3 wo = neg(normalize(dx * U + dy * V + W));
                Np = normalize(cross(B - A, Cc - A)) * copysignf(1.0f, dot(wo, N_0));
            }
            v = Xp - v3(a.eye_prev[0], a.eye_prev[1], a.eye_prev[2]);
        } else {                                                           // k_gbuffer_rays' direction, before normalising
            const float dx = 2.0f * (((float)x + 0.5f) / (float)fd.w) - 1.0f;
            const float dy = 2.0f * (((float)y + 0.5f) / (float)fd.h) - 1.0f;
            const V3 U = v3(fd.U[0], fd.U[1], fd.U[2]), V = v3(fd.V[0], fd.V[1], fd.V[2]), W = v3(fd.W[0], fd.W[1], fd.W[2]);
            v = dx * U + dy * V + W;
        }
        const float ax = (a.inv[0] * v.x + a.inv[1] * v.y) + a.inv[2] * v.z;
        const float ay = (a.inv[3] * v.x + a.inv[4] * v.y) + a.inv[5] * v.z;
        const float az = (a.inv[6] * v.x + a.inv[7] * v.y) + a.inv[8] * v.z;
        if (az > 0.0f) {
            const float fw = (float)fd.w, fh = (float)fd.h;
            const float px = (((ax / az) + 1.0f) * 0.5f) * fw - 0.5f;
            const float py = (((ay / az) + 1.0f) * 0.5f) * fh - 0.5f;
            if (px >= -1.0f && px < fw && py >= -1.0f && py < fh) {        // (NaN fails): x0 in [-1, w - 1], y0 in [-1, h - 1]
                mv = make_float4(px - (float)x, py - (float)y, az, 1.0f);
                if (cap > 1) {
                    const float x0f = floorf(px), y0f = floorf(py);
                    const float fx = px - x0f, fy = py - y0f;
                    const int x0 = (int)x0f, y0 = (int)y0f;
                    const float wt[4] = {(1.0f - fx) * (1.0f - fy), fx * (1.0f - fy), (1.0f - fx) * fy, fx * fy};
                    const float ztol = a.depth_tol * xp4.w;
                    float sw = 0.0f, sn = 0.0f;
                    V3 acc = v3(0.0f);
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
                        if (qx < 0 || qx >= fd.w || qy < 0 || qy >= fd.h) continue;
                        const uint32_t q = (uint32_t)qy * (uint32_t)fd.w + (uint32_t)qx;
                        if ((gp.prim[q] == 0xffffffffu) != miss_p) continue;
                        if (!miss_p) {
                            const V3 Nq = v3(gp.nrm[q]), Xq = v3(gp.pos[q]);
                            if (!(sq3(Nq - Np) <= a.normal_tol)) continue;           // (a degenerate previous triangle: N' is not finite)
                            if (!(fabsf(dot(Np, Xq - Xp)) <= ztol)) continue;
                        }
                        const float4 hq = hist_prev[q];
                        sw = sw + wt[k];
                        acc = acc + v3(hq) * wt[k];
                        sn = sn + hq.w * wt[k];
                    }
                    if (sw >= 1.0f / 64.0f) {
                        H = v3(acc.x / sw, acc.y / sw, acc.z / sw);
                        nh = sn / sw;
                    }
                }
            }
        }
    }
    if (want_motion) m.out_motion[idx] = fovpt_float4{mv.x, mv.y, mv.z, mv.w};
    const float n = fminf(nh + 1.0f, (float)cap);
    if (n == 1.0f) {                                                       // first step, disocclusion, cap 1: the input, bit for bit
        out_color[idx] = c;
        hist_out[idx] = make_float4(c.x, c.y, c.z, 1.0f);
        out_rgba[idx] = make_color(reinhard(v3(c.x, c.y, c.z) * 16.0f, 1.0f));
        return;
    }
    const V3 o = lerp3(H, v3(c.x, c.y, c.z), 1.0f / n);
    out_color[idx] = fovpt_float4{o.x, o.y, o.z, 1.0f};
    hist_out[idx] = f4(o, n);
    out_rgba[idx] = make_color(reinhard(o * 16.0f, 1.0f));
}

}  // namespace

void fovpt_launch_temporal_motion(hipStream_t st, const FrameDev& fd, const TemporalArgs& a, const TemporalMotionArgs& m, const fovpt_float4* in,
                                  GBufferDev g, GBufferDev gp, const float4* hist_prev, float4* hist_out, fovpt_float4* out_color,
                                  uint32_t* out_rgba)
{
    const dim3 grid((fd.w + 63) / 64, (fd.h + 3) / 4);
    hipLaunchKernelGGL(k_temporal_motion, grid, dim3(FOVPT_BLOCK), 0, st, fd, a, m, in, g, gp, hist_prev, hist_out, out_color, out_rgba);
}

void fovpt_launch_temporal(hipStream_t st, const FrameDev& fd, const TemporalArgs& a, const fovpt_float4* in, GBufferDev g, GBufferDev gp,
                           const float4* hist_prev, float4* hist_out, fovpt_float4* out_color, uint32_t* out_rgba)
{
    const dim3 grid((fd.w + 63) / 64, (fd.h + 3) / 4);
    hipLaunchKernelGGL(k_temporal, grid, dim3(FOVPT_BLOCK), 0, st, fd, a, in, g, gp, hist_prev, hist_out, out_color, out_rgba);
}
