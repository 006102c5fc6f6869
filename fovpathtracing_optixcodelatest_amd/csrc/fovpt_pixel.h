// fovpt_pixel.h -- device helpers of anything that works on a frame's pixels: the wavefront kernels (wavefront.hip) and every
// post-frame stage.  The fp32 vector type, a thread's pixel in the 64 x 4 tiling, the ring test, the resolve's tone map and its
// store, Rec. 709 luminance, the last-writer search over a frame's passes and the pick of a per-level value by the writer's fill.
// What only post-frame stages share is in fovpt_post_pixel.h.
#pragma once

#include "fovpt_device.h"
#include "../../include/fovpt_detmath.h"

namespace {

// ------------------------------------------------------------------------------------------
// fp32 vector helpers with the semantics of sutil/vec_math.h
// ------------------------------------------------------------------------------------------
struct V3 { float x, y, z; };
__device__ inline V3 v3(float x, float y, float z) { V3 r = {x, y, z}; return r; }
__device__ inline V3 v3(float s) { return v3(s, s, s); }
__device__ inline V3 v3(const float4& a) { return v3(a.x, a.y, a.z); }
__device__ inline V3 v3(const fovpt_float3& a) { return v3(a.x, a.y, a.z); }
__device__ inline V3 v3(const fovpt_float4& a) { return v3(a.x, a.y, a.z); }
__device__ inline V3 neg(const V3& a) { return v3(-a.x, -a.y, -a.z); }
__device__ inline V3 operator+(const V3& a, const V3& b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ inline V3 operator-(const V3& a, const V3& b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ inline V3 operator*(const V3& a, const V3& b) { return v3(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ inline V3 operator*(const V3& a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
__device__ inline V3 operator*(float s, const V3& a) { return v3(a.x * s, a.y * s, a.z * s); }
__device__ inline V3 sub_sv(float a, const V3& b) { return v3(a - b.x, a - b.y, a - b.z); }          // float - float3
__device__ inline V3 add_vs(const V3& a, float b) { return v3(a.x + b, a.y + b, a.z + b); }          // float3 + float
__device__ inline V3 div_vs(const V3& a, float s) { float inv = 1.0f / s; return a * inv; }          // vec_math.h:487
__device__ inline float dot(const V3& a, const V3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline V3 cross(const V3& a, const V3& b)
{ return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
__device__ inline V3 normalize(const V3& v) { float invLen = 1.0f / sqrtf(dot(v, v)); return v * invLen; }
__device__ inline float clampf(float f, float a, float b) { return fmaxf(a, fminf(f, b)); }
__device__ inline V3 clamp3(const V3& v, float a, float b) { return v3(clampf(v.x, a, b), clampf(v.y, a, b), clampf(v.z, a, b)); }
__device__ inline float lerpf(float a, float b, float t) { return a + t * (b - a); }
__device__ inline V3 lerp3(const V3& a, const V3& b, float t) { return a + t * (b - a); }
__device__ inline float sqr(float a) { return a * a; }
__device__ inline float4 f4(const V3& a, float w) { return make_float4(a.x, a.y, a.z, w); }

// The pixel (x, y) and its index of the calling thread where a block is a 64 x 4 tile of a w x h image (the grid: fovpt_tile_grid);
// false outside the image.  T: the coordinates' type, int or uint32_t, as the kernel's arithmetic on them wants.
template <class T>
__device__ inline bool tile_pixel(int w, int h, T& x, T& y, uint32_t& idx)
{
    x = (T)(blockIdx.x * FOVPT_TILE_W + threadIdx.x % FOVPT_TILE_W);
    y = (T)(blockIdx.y * FOVPT_TILE_H + threadIdx.x / FOVPT_TILE_W);
    idx = (uint32_t)y * (uint32_t)w + (uint32_t)x;
    return x < (T)w && y < (T)h;
}

// ring test of deviceProgram.cu:433-440 on the block's top-left pixel (uint arithmetic wraps)
__device__ inline bool ring_alive(const FrameDev& fd, const PassDev& P, uint32_t lx, uint32_t ly, uint32_t& ix, uint32_t& iy)
{
    ix = lx * P.fx + P.offx;
    iy = ly * P.fy + P.offy;
    const float dx = (float)ix - (float)fd.cx, dy = (float)iy - (float)fd.cy, dz = 0.0f - 0.0f;
    const float range = sqrtf(dx * dx + dy * dy + dz * dz);
    return !(range < P.r_inner || range > P.r_outer);
}

// ---- tone map of the resolve ---------------------------------------------------------------
__device__ inline float luma(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }   // Rec. 709
__device__ inline float luma(const V3& c) { return luma(c.x, c.y, c.z); }
__device__ inline V3 reinhard(const V3& color, float white)                    // :126-131
{
    return div_vs(color * 1.0f, 1.0f + luma(color) / white);
}
__device__ inline float srgb1(float c)                                          // cuda/helpers.h:35-43
{
    const float invGamma = 1.0f / 2.4f;
    const float powed = fovpt_dm_powf(c, invGamma);
    return c < 0.0031308f ? 12.92f * c : 1.055f * powed - 0.055f;
}
__device__ inline uint32_t quant8(float x)                                      // cuda/helpers.h:50-55
{
    x = clampf(x, 0.0f, 1.0f);
    return min((uint32_t)(x * 256.0f), 255u);
}
__device__ inline uint32_t make_color(const V3& c)                              // cuda/helpers.h:57-62
{
    const V3 cc = clamp3(c, 0.0f, 1.0f);
    return quant8(srgb1(cc.x)) | (quant8(srgb1(cc.y)) << 8) | (quant8(srgb1(cc.z)) << 16) | (255u << 24);
}
// a post-frame stage's outputs as the resolve stores a pixel: the rgba8 of colour c, and c with w = 1 beside it
__device__ inline uint32_t resolved_rgba(const V3& c) { return make_color(reinhard(c * 16.0f, 1.0f)); }
__device__ inline void store_resolved(fovpt_float4* out_color, uint32_t* out_rgba, uint32_t idx, const V3& c)
{
    out_color[idx] = fovpt_float4{c.x, c.y, c.z, 1.0f};
    out_rgba[idx] = resolved_rgba(c);
}

// ---- last writer of a pixel -----------------------------------------------------------------
// candidate launch-index range along one axis for pixel coordinate x (resolve)
// `wrap` (>= 0 only on the clamped edge): launch indices 0 .. wrap have a "negative" pixel index, which in the
// reference's unsigned arithmetic is a huge one and is clamped onto this edge too (deviceProgram.cu:433, :554).
// They only ever pass the ring test when the gaze point itself is such a wrapped coordinate.
__device__ inline void writer_range(uint32_t x, uint32_t frame_dim, uint32_t factor, int fill, uint32_t off, uint32_t grid, long long& lo, long long& hi,
                                    long long& wrap)
{
    // r = x - (int32)off, a = max(0, ceil((r - (fill-1)) / f)), b = floor(r / f) (or grid-1 on the clamped edge).
    // Integer division is a long software routine on the GPU: power-of-two factors (1, 2, 4 in every
    // pass the reference launches) shift, everything else that fits uses 32-bit division.
    const long long r = (long long)x - (long long)(int32_t)off;
    const uint32_t f = factor ? factor : 1u;
    const bool pow2 = (f & (f - 1u)) == 0u;
    const int sh = 31 - __clz((int)f);
    const long long num = r - (long long)(fill - 1);          // a = ceil(num / f)
    long long a;
    if (num <= 0) a = 0;
    else if (num < 0x7fffffffll) a = pow2 ? (long long)(((uint32_t)num + f - 1u) >> sh) : (long long)(((uint32_t)num + f - 1u) / f);
    else a = (num + f - 1) / (long long)f;
    long long b;
    if (x + 1 == frame_dim) b = (long long)grid - 1;  // clamp at :554 folds everything beyond the edge onto it
    else {
        if (r < 0) b = -1;
        else if (r < 0x7fffffffll) b = pow2 ? (long long)((uint32_t)r >> sh) : (long long)((uint32_t)r / f);
        else b = r / (long long)f;
        if (b > (long long)grid - 1) b = (long long)grid - 1;
    }
    lo = a; hi = b;
    wrap = -1;
    if (x + 1 == frame_dim && (int32_t)off < 0) {
        const long long neg = -(long long)(int32_t)off;                       // index of launch l is l*f - neg
        long long cnt = (neg + (long long)f - 1) / (long long)f;              // l*f < neg
        if (cnt > (long long)grid) cnt = grid;
        wrap = cnt - 1;
        if (wrap >= lo) wrap = lo - 1;                                        // (already part of [lo, hi])
    }
}

// The last writer of pixel (x, y) in the reference's launch order: the highest pass that covers it (F over M over P),
// within a pass the launch index that comes last (ascending y, then x) among those whose clamped block fill reaches the
// pixel (deviceProgram.cu:546-554) and that pass the ring test (:433-440).  Only launch rows [row0, row1) of a pass count
// (a chunk of a large launch).  Used by the resolve and by the multi-GPU gather plan.
__device__ inline bool find_last_writer(const FrameDev& fd, uint32_t x, uint32_t y, int& wp, uint32_t& wlx, uint32_t& wly)
{
#pragma unroll
    for (int p = FOVPT_MAX_PASSES - 1; p >= 0; p--) {          // static indices: the pass records stay in SGPRs
        if (p >= fd.npass) continue;
        const PassDev& P = fd.pass[p];
        if (P.fill <= 0) continue;
        // The common case first (round 4; the general search below is ~800 instructions per pixel, most of a resolve's time):
        // blocks that tile the plane -- fill == factor, a power of two, as in every pass the reference launches -- have, away
        // from the frame's last column and row (where the clamp at :554 folds launches onto the edge), exactly ONE candidate
        // per axis: a = ceil((r - f + 1) / f) = floor(r / f) = b.
        const uint32_t f = P.fx;
        if ((uint32_t)P.fill == f && P.fy == f && (f & (f - 1u)) == 0u && x + 1u != (uint32_t)fd.w && y + 1u != (uint32_t)fd.h) {
            const int sh = 31 - __clz((int)f);
            const long long rx = (long long)x - (long long)(int32_t)P.offx, ry = (long long)y - (long long)(int32_t)P.offy;
            if (rx < 0 || ry < 0 || rx >= ((long long)P.gw << sh) || ry >= ((long long)P.row1 << sh)) continue;
            const uint32_t lx = (uint32_t)rx >> sh, ly = (uint32_t)ry >> sh;
            uint32_t ix, iy;
            if (ly < P.row0 || !ring_alive(fd, P, lx, ly, ix, iy)) continue;
            wp = p; wlx = lx; wly = ly;
            return true;
        }
        long long xa, xb, ya, yb, xw, yw;
        writer_range(x, (uint32_t)fd.w, P.fx, P.fill, P.offx, P.gw, xa, xb, xw);
        writer_range(y, (uint32_t)fd.h, P.fy, P.fill, P.offy, P.gh, ya, yb, yw);
        if (ya < (long long)P.row0) ya = P.row0;           // only this chunk's launch rows
        if (yb > (long long)P.row1 - 1) yb = (long long)P.row1 - 1;
        if (yw > (long long)P.row1 - 1) yw = (long long)P.row1 - 1;
        const long long y_end = yw >= (long long)P.row0 ? (long long)P.row0 : ya, x_end = xw >= 0 ? 0 : xa;
        // candidates in descending launch order: [ya, yb] then the wrapped rows [row0, yw]; same along x
        for (long long ly = yb; ly >= y_end; ly--) {
            if (ly < ya && ly > yw) { ly = yw + 1; continue; }
            for (long long lx = xb; lx >= x_end; lx--) {
                if (lx < xa && lx > xw) { lx = xw + 1; continue; }
                uint32_t ix, iy;
                if (!ring_alive(fd, P, (uint32_t)lx, (uint32_t)ly, ix, iy)) continue;
                wp = p; wlx = (uint32_t)lx; wly = (uint32_t)ly;
                return true;
            }
        }
    }
    return false;
}

// a per-level value for a pixel whose last writer has fill f: t = {fill 1, fill 2, fill 4, FOV_OFF}
template <class T>
__device__ inline T by_level(const T (&t)[4], bool uniform, int f)
{
    const T t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3];       // (all four read first: the pick is selects, no branch)
    return uniform ? t3 : f == 4 ? t2 : f == 2 ? t1 : t0;
}

}  // namespace
