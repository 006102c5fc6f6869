// fovpt_post_pixel.h -- what the post-frame stages share beyond fovpt_pixel.h, each step in one place:
//   - albedo demodulation and the edge-stopping terms (demod, div3, sq3, edge) of the denoiser, the reconstruction and the
//     variance-guided filter;
//   - the a-trous filters' level byte, B3 weights and clamped taps (denoise.hip, variance.hip);
//   - the projection of a point or direction into another camera's pixels (temporal.hip, warp.hip);
//   - the per-pixel bodies of the reconstruction and of the temporal step: k_reconstruct (reconstruct.hip), k_temporal /
//     k_temporal_motion (temporal.hip) and k_reconstruct_temporal (post_fused.hip) are these functions between their loads of the
//     input pixel and their stores.  Their definitions, operation by operation, are tests/reconstruct_ref.py,
//     tests/temporal_ref.py and tests/temporal_motion_ref.py.
// -ffp-contract=off keeps every product and sum a separate binary32 op.
//
// A pixel's own G-buffer entry reaches the bodies through an accessor (prim() / pos() / nrm()): GLazy reads memory where the
// body asks, which is where the separate kernels always read it; GRegs holds an entry that the fused kernel has read once.
#pragma once

#include "fovpt_device.h"
#include "fovpt_pixel.h"

namespace {

struct GLazy {
    const GBufferDev& g;
    uint32_t idx;
    __device__ inline uint32_t prim() const { return g.prim[idx]; }
    __device__ inline float4 pos() const { return g.pos[idx]; }
    __device__ inline float4 nrm() const { return g.nrm[idx]; }
};
struct GRegs {
    uint32_t prim_;
    float4 pos_, nrm_;
    __device__ inline uint32_t prim() const { return prim_; }
    __device__ inline float4 pos() const { return pos_; }
    __device__ inline float4 nrm() const { return nrm_; }
};

// ---- demodulation and edge stopping ----------------------------------------------------------
__device__ inline V3 demod(const V3& a)                                    // the albedo to divide by: never below 1 / 64, 1 where black
{
    const float s = a.x + a.y + a.z;
    if (s > 0.0f) return v3(fmaxf(a.x, 1.0f / 64.0f), fmaxf(a.y, 1.0f / 64.0f), fmaxf(a.z, 1.0f / 64.0f));
    return v3(1.0f);
}
__device__ inline float edge(float d) { const float t = fmaxf(0.0f, 1.0f - d); return t * t; }
__device__ inline float sq3(const V3& a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
__device__ inline V3 div3(const V3& a, const V3& b) { return v3(a.x / b.x, a.y / b.y, a.z / b.z); }
__device__ inline V3 div3(const V3& a, float s) { return v3(a.x / s, a.y / s, a.z / s); }       // (three divisions: not div_vs)

// ---- a-trous filters ---------------------------------------------------------------------------
// A pixel's level: the iterations n of its last writer's pass and log2 of that pass's fill (1, 2, 4), kept between the prep and
// the step kernels as one byte, n in bits 0-3 and the shift in bits 4-7.
struct AtrousLevel {
    int n, fill_shift;
    __device__ inline uint8_t code() const { return (uint8_t)(n | (fill_shift << 4)); }
};
__device__ inline AtrousLevel atrous_decode(int code) { return AtrousLevel{code & 15, code >> 4}; }
// the level of pixel (x, y): n_pass[p] iterations where pass p writes it last, 0 where no pass does
__device__ inline AtrousLevel atrous_level(const FrameDev& fd, const int32_t* n_pass, uint32_t x, uint32_t y)
{
    int wp = 0;
    AtrousLevel l = {0, 0};
    uint32_t wlx, wly;
    if (find_last_writer(fd, x, y, wp, wlx, wly)) {
        l.n = n_pass[wp];
        l.fill_shift = 31 - __clz(fd.pass[wp].fill);
    }
    return l;
}
// B3-spline weight of tap d = -2 .. 2 along an axis: b3_weight where d is a constant once its loop is unrolled, b3_weight_row where
// it is a run-time value (compares: indexing the table would be a memory lookup per tap row)
__device__ inline float b3_weight(int d)
{
    const float H[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    return H[d + 2];
}
__device__ inline float b3_weight_row(int d) { return d == 0 ? 3.0f / 8.0f : (d == 1 || d == -1) ? 1.0f / 4.0f : 1.0f / 16.0f; }
// tap d at step s from coordinate p of an axis of n pixels, clamped to the image
__device__ inline int tap_coord(int p, int s, int d, int n) { return min(max(p + s * d, 0), n - 1); }

// ---- projection into another camera ----------------------------------------------------------
// v (a point relative to that camera's eye, or a direction) in the camera whose inverse [U V W]^-1 has the rows inv: its depth
// az along W and, meaningful where az > 0, its position (px, py) in pixels of an fw x fh image
__device__ inline void project(const float* inv, const V3& v, float fw, float fh, float& az, float& px, float& py)
{
    const float ax = (inv[0] * v.x + inv[1] * v.y) + inv[2] * v.z;
    const float ay = (inv[3] * v.x + inv[4] * v.y) + inv[5] * v.z;
    az = (inv[6] * v.x + inv[7] * v.y) + inv[8] * v.z;
    px = (((ax / az) + 1.0f) * 0.5f) * fw - 0.5f;
    py = (((ay / az) + 1.0f) * 0.5f) * fh - 0.5f;
}

// ---- reconstruction and temporal step --------------------------------------------------------

// whether the reconstruction is on for a pixel whose last writer has fill f
__device__ inline bool reconstruct_level_on(const ReconstructArgs& a, int f) { return f > 1 && (a.levels & (f == 2 ? 1 : 2)); }

// The reconstruction of pixel (x, y), last written by launch (wlx, wly) of pass wp: true and its colour in o, or false where
// the pixel keeps its input (fill 1, its level masked, or weights that sum to 0).
template <class G>
__device__ inline bool reconstruct_pixel(const FrameDev& fd, const ReconstructArgs& a, const fovpt_float4* __restrict__ in,
                                         const fovpt_float4* __restrict__ albedo, const GBufferDev& g, const G& own, uint32_t x, uint32_t y,
                                         uint32_t idx, int wp, uint32_t wlx, uint32_t wly, V3& o)
{
    const PassDev& P = fd.pass[wp];
    const int f = P.fill;
    if (reconstruct_level_on(a, f)) {
        uint32_t ix, iy;
        (void)ring_alive(fd, P, wlx, wly, ix, iy);                      // the anchor: the block's sample pixel (may wrap)
        const float inv_s = a.inv_support[f == 2 ? 0 : 1];
        const bool miss_p = own.prim() == 0xffffffffu;
        const float4 xp4 = own.pos(), np4 = own.nrm();
        const V3 Xp = v3(xp4), Np = v3(np4);
        const float tp2 = xp4.w * xp4.w;
        const long long w1 = fd.w - 1, h1 = fd.h - 1;
        float sw = 0.0f;
        V3 acc = v3(0.0f);
#pragma unroll
        for (int j = -1; j <= 1; j++) {
            const long long qy = min(max((long long)iy + (long long)(j * f), 0ll), h1);
            const float hy = fmaxf(0.0f, 1.0f - fabsf((float)((long long)y - qy)) * inv_s);
#pragma unroll
            for (int i = -1; i <= 1; i++) {
                const long long qx = min(max((long long)ix + (long long)(i * f), 0ll), w1);
                const float hx = fmaxf(0.0f, 1.0f - fabsf((float)((long long)x - qx)) * inv_s);
                const uint32_t q = (uint32_t)qy * (uint32_t)fd.w + (uint32_t)qx;
                const bool miss_q = g.prim[q] == 0xffffffffu;
                float wn = 1.0f, wz = 1.0f;
                if (miss_p != miss_q) wn = wz = 0.0f;
                else if (!miss_p) {
                    const V3 Nq = v3(g.nrm[q]), Xq = v3(g.pos[q]);
                    wn = edge(sq3(Nq - Np) * a.inv_n);
                    const float dz = dot(Np, Xq - Xp);
                    wz = edge(((dz * dz) * a.inv_z) / tp2);
                }
                const float wt = ((hx * hy) * wn) * wz;
                const fovpt_float4 cq = in[q];
                V3 Iq = v3(cq);
                if (a.remodulate) {
                    const fovpt_float4 aq = albedo[q];
                    Iq = div3(Iq, demod(v3(aq)));
                }
                sw = sw + wt;
                acc = acc + Iq * wt;
            }
        }
        if (sw > 0.0f) {
            o = div3(acc, sw);
            if (a.remodulate) o = o * demod(v3(g.alb[idx]));
            return true;
        }
    }
    return false;
}

// the history cap of a pixel: by the fill of its last writer (found: pass wp), 1 where no pass writes
__device__ inline int history_cap(const FrameDev& fd, const TemporalArgs& a, bool found, int wp)
{
    if (!found) return 1;
    const int f = fd.pass[wp].fill;                                         // (not by_level: with it k_reconstruct_temporal needs 4 more SGPRs)
    return a.uniform ? a.cap[3] : f == 4 ? a.cap[2] : f == 2 ? a.cap[1] : a.cap[0];
}

// k_gbuffer_rays' direction of pixel (x, y), before normalising
__device__ inline V3 pixel_ray(const FrameDev& fd, uint32_t x, uint32_t y)
{
    const float dx = 2.0f * (((float)x + 0.5f) / (float)fd.w) - 1.0f;
    const float dy = 2.0f * (((float)y + 0.5f) / (float)fd.h) - 1.0f;
    const V3 U = v3(fd.U[0], fd.U[1], fd.U[2]), V = v3(fd.V[0], fd.V[1], fd.V[2]), W = v3(fd.W[0], fd.W[1], fd.W[2]);
    return dx * U + dy * V + W;
}

// The four bilinear taps of the previous history around (px, py), kept where the previous G-buffer agrees with the pixel's
// class, normal Np and point Xp: H and nh where enough weight remains.
__device__ inline void history_taps(const FrameDev& fd, const TemporalArgs& a, const GBufferDev& gp, const float4* __restrict__ hist_prev,
                                    float px, float py, bool miss_p, const V3& Xp, const V3& Np, float ztol, V3& H, float& nh)
{
    const float x0f = floorf(px), y0f = floorf(py);
    const float fx = px - x0f, fy = py - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const float wt[4] = {(1.0f - fx) * (1.0f - fy), fx * (1.0f - fy), (1.0f - fx) * fy, fx * fy};
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
            if (!(sq3(Nq - Np) <= a.normal_tol)) continue;                   // (a degenerate previous triangle: N' is not finite)
            if (!(fabsf(dot(Np, Xq - Xp)) <= ztol)) continue;
        }
        const float4 hq = hist_prev[q];
        sw = sw + wt[k];
        acc = acc + v3(hq) * wt[k];
        sn = sn + hq.w * wt[k];
    }
    if (sw >= 1.0f / 64.0f) {
        H = div3(acc, sw);
        nh = sn / sw;
    }
}

// k_temporal's history of pixel (x, y) with cap `cap`: H and nh (left as they are where the pixel does not reproject)
template <class G>
__device__ inline void temporal_history(const FrameDev& fd, const TemporalArgs& a, const G& own, const GBufferDev& gp,
                                        const float4* __restrict__ hist_prev, uint32_t x, uint32_t y, int cap, V3& H, float& nh)
{
    if (a.reproject && cap > 1) {                                          // (cap 1: n is 1 whatever the history says)
        const bool miss_p = own.prim() == 0xffffffffu;
        const float4 xp4 = own.pos();
        const V3 Xp = v3(xp4);
        V3 v;
        if (!miss_p) v = Xp - v3(a.eye_prev[0], a.eye_prev[1], a.eye_prev[2]);
        else v = pixel_ray(fd, x, y);
        const float fw = (float)fd.w, fh = (float)fd.h;
        float az, px, py;
        project(a.inv, v, fw, fh, az, px, py);
        if (az > 0.0f && px >= -1.0f && px < fw && py >= -1.0f && py < fh) {   // (NaN fails): x0 in [-1, w - 1], y0 in [-1, h - 1]
            const V3 Np = v3(own.nrm());
            history_taps(fd, a, gp, hist_prev, px, py, miss_p, Xp, Np, a.depth_tol * xp4.w, H, nh);
        }
    }
}

// The previous positions a', b', c' of primitive prim's vertices (tri_vidx: its index triple into vtx_prev), and the point
// X' = (w0 a' + u b') + v c', w0 = (1 - u) - v, of a hit record (t, u, v, record) over them: what fovpt_temporal_motion and
// fovpt_warp_motion take for where a moved surface was at the previous step.
__device__ inline void previous_vertices(const uint3* tri_vidx, const float* vtx_prev, uint32_t prim, V3& A, V3& B, V3& Cc)
{
    const uint3 iv = tri_vidx[prim];
    const float* pa = vtx_prev + 3 * (size_t)iv.x, *pb = vtx_prev + 3 * (size_t)iv.y, *pc = vtx_prev + 3 * (size_t)iv.z;
    A = v3(pa[0], pa[1], pa[2]); B = v3(pb[0], pb[1], pb[2]); Cc = v3(pc[0], pc[1], pc[2]);
}
__device__ inline V3 previous_point(const float4& hit, const V3& A, const V3& B, const V3& Cc)
{
    const float w0 = (1.0f - hit.y) - hit.z;
    return (w0 * A + hit.y * B) + hit.z * Cc;
}

// k_temporal_motion's: temporal_history in which a hit pixel whose mesh is marked (m.mark[mesh] == m.epoch) gets
// X' = (w0 a' + u b') + v c' and N' = normalize(cross(b' - a', c' - a')) * s from its triangle's previous vertices a', b', c' and
// its hit's (u, v), s the sign k_gbuffer_fill gave the current normal; every other pixel takes temporal_history's operations.
// The common case -- an unmarked mesh -- pays for the hit record's last word, one word of the triangle record and the mark,
// not for the vertex gathers.  With want_motion the projection also runs for cap-1 pixels and mv becomes (px - x, py - y, a.z, 1)
// where the pixel reprojects.
template <class G>
__device__ inline void temporal_motion_history(const FrameDev& fd, const TemporalArgs& a, const TemporalMotionArgs& m, const G& own,
                                               const GBufferDev& gp, const float4* __restrict__ hist_prev, uint32_t x, uint32_t y,
                                               uint32_t idx, int cap, bool want_motion, V3& H, float& nh, float4& mv)
{
    if (a.reproject && (cap > 1 || want_motion)) {
        const uint32_t prim = own.prim();
        const bool miss_p = prim == 0xffffffffu;
        const float4 xp4 = own.pos();
        V3 Xp = v3(xp4), Np = v3(0.0f);
        V3 v;
        if (!miss_p) {
            Np = v3(own.nrm());
            const uint32_t rec = __float_as_uint(m.hit[idx].w) << 4;       // byte offset of the triangle record, as k_gbuffer_fill's
            const float4* tr = (const float4*)((const char*)m.tris + rec);
            const uint32_t mesh = __float_as_uint(tr[2].z);
            if (m.mark[mesh] == m.epoch) {
                const float4 hit = m.hit[idx];
                V3 A, B, Cc;
                previous_vertices(m.tri_vidx, m.vtx_prev, prim, A, B, Cc);
                Xp = previous_point(hit, A, B, Cc);
                // s: k_gbuffer_fill's copysignf(1, dot(wo, N_0)) over the current record's edges and k_gbuffer_rays' direction
                const float4 t0 = tr[0], t1 = tr[1];
                const V3 N_0 = normalize(cross(v3(t0.w, t1.x, t1.y), v3(t1.z, t1.w, tr[2].x)));
                const V3 wo = neg(normalize(pixel_ray(fd, x, y)));
                Np = normalize(cross(B - A, Cc - A)) * copysignf(1.0f, dot(wo, N_0));
            }
            v = Xp - v3(a.eye_prev[0], a.eye_prev[1], a.eye_prev[2]);
        } else v = pixel_ray(fd, x, y);
        const float fw = (float)fd.w, fh = (float)fd.h;
        float az, px, py;
        project(a.inv, v, fw, fh, az, px, py);
        if (az > 0.0f && px >= -1.0f && px < fw && py >= -1.0f && py < fh) {   // (NaN fails): x0 in [-1, w - 1], y0 in [-1, h - 1]
            mv = make_float4(px - (float)x, py - (float)y, az, 1.0f);
            if (cap > 1) history_taps(fd, a, gp, hist_prev, px, py, miss_p, Xp, Np, a.depth_tol * xp4.w, H, nh);
        }
    }
}

// the blend and the three stores of a temporal step: out = lerp(H, c, 1 / n), n = min(nh + 1, cap), the new history (out, n)
__device__ inline void temporal_blend(const fovpt_float4& c, const V3& H, float nh, int cap, uint32_t idx, float4* __restrict__ hist_out,
                                      fovpt_float4* out_color, uint32_t* __restrict__ out_rgba)
{
    const float n = fminf(nh + 1.0f, (float)cap);
    if (n == 1.0f) {                                                       // first step, disocclusion, cap 1: the input, bit for bit
        out_color[idx] = c;
        hist_out[idx] = make_float4(c.x, c.y, c.z, 1.0f);
        out_rgba[idx] = resolved_rgba(v3(c));                              // (c keeps its own w: not store_resolved)
        return;
    }
    const V3 o = lerp3(H, v3(c), 1.0f / n);
    hist_out[idx] = f4(o, n);
    store_resolved(out_color, out_rgba, idx, o);
}

}  // namespace
