// warp.hip -- fovpt_warp: late reprojection of a finished frame to a newer camera.  fovpt_temporal pulls
// old colours into a frame whose depth is known: a gather.  Here only the OLD frame's depth is known, so the pixels are pushed:
//
//   k_warp_scatter   per source pixel: its G-buffer point (a hit) or its camera-ray direction (a miss) projected into the `to`
//                    camera with fovpt_temporal's expression (project, fovpt_post_pixel.h), rounded to the nearest pixel, and one
//                    64-bit atomic minimum of (depth bits << 32 | source index) on that pixel's key.  Nearest depth wins, equal
//                    depths go to the lower source index: the keys do not depend on the order in which the atomics arrive
//   k_warp_scatter_motion   fovpt_warp_motion's scatter: k_warp_scatter in which a hit pixel of a mesh that moved in the last
//                    interval lands where its own motion, extrapolated by `advance` intervals, takes it
//   k_warp_scatter_depth    fovpt_warp_depth's scatter: k_warp_scatter with the source point rebuilt from a depth image and the
//                    camera it was rendered with, for a client that holds no scene
//   k_warp_resolve   per destination pixel: the key's source; for an empty key the farthest key of the nearest non-empty
//                    Chebyshev ring within fill_radius; else the pixel itself.  Copies the enabled images from the source,
//                    bit for bit, and writes the map
//
// One thread per pixel, 64 x 4 pixel tiles (a wave is 64 pixels of a row), no LDS.  The four counts are per wave: a ballot, a
// popcount and one atomic add by the wave's first lane, into one of 256 copies of the record that the host adds up.  The
// definition, operation by operation, is tests/warp_ref.py; -ffp-contract=off keeps every product and sum of it a separate
// binary32 op.
#include "fovpt_device.h"
#include "fovpt_pixel.h"
#include "fovpt_post_pixel.h"

namespace {

#define WARP_EMPTY 0xffffffffffffffffull

// The counts record of this wave: one of FOVPT_WARP_COUNT_SLOTS copies, FOVPT_WARP_COUNT_STRIDE words apart (the host adds
// them up).  With one copy every wave of the frame adds to the same four words, and those atomics are carried out one after
// the other: at 1920 x 1080 that was 0.9 ms of a call.
__device__ inline unsigned long long* count_slot(unsigned long long* counts)
{
    const uint32_t wave = (blockIdx.y * gridDim.x + blockIdx.x) * (FOVPT_BLOCK / FOVPT_WAVE) + threadIdx.x / FOVPT_WAVE;
    return counts + (size_t)(wave % FOVPT_WARP_COUNT_SLOTS) * FOVPT_WARP_COUNT_STRIDE;
}

// lanes of the wave for which p holds, counted once into *n (every lane of the wave calls this)
__device__ inline void count_wave(bool p, unsigned long long* n)
{
    const unsigned long long m = __ballot(p);
    if ((threadIdx.x & (FOVPT_WAVE - 1)) == 0 && m) atomicAdd(n, (unsigned long long)__popcll(m));
}

// The tail of a scatter: v (source pixel s's point relative to the `to` eye, or a miss's direction) projected with fovpt_temporal's
// expression, rounded to the nearest pixel, and the atomic minimum on that pixel's key.  false: it lands outside the frame or behind
// the camera
__device__ inline bool scatter_key(const FrameDev& fd, const WarpArgs& a, const V3& v, bool miss, uint32_t s,
                                   unsigned long long* __restrict__ keys)
{
    const float fw = (float)fd.w, fh = (float)fd.h;
    float az, px, py;
    project(a.inv, v, fw, fh, az, px, py);
    const float fx = floorf(px + 0.5f), fy = floorf(py + 0.5f);
    const bool landed = az > 0.0f && fx >= 0.0f && fx < fw && fy >= 0.0f && fy < fh;   // (in float, before converting: NaN fails)
    if (landed) {
        const uint32_t d = miss ? 0x7fffffffu : __float_as_uint(az);      // (az > 0: its bits order as its value does)
        const uint32_t q = (uint32_t)fy * (uint32_t)fd.w + (uint32_t)fx;
        (void)atomicMin(&keys[q], ((unsigned long long)d << 32) | (unsigned long long)s);
    }
    return landed;
}

__global__ __launch_bounds__(FOVPT_BLOCK) void k_warp_scatter(const FrameDev fd, const WarpArgs a, const uint32_t* __restrict__ prim,
                                                              const float4* __restrict__ pos, unsigned long long* __restrict__ keys,
                                                              unsigned long long* __restrict__ counts)
{
    uint32_t x, y, s;
    bool landed = false;
    if (tile_pixel(fd.w, fd.h, x, y, s)) {                                // (lanes outside the frame go on to count_wave)
        const bool miss = prim[s] == 0xffffffffu;
        V3 v;
        if (!miss) v = v3(pos[s]) - v3(a.eye[0], a.eye[1], a.eye[2]);
        else v = pixel_ray(fd, x, y);                                    // the sky is at infinity: only rotation moves it
        landed = scatter_key(fd, a, v, miss, s, keys);
    }
    count_wave(landed, &count_slot(counts)[0]);
}

// fovpt_warp_motion's scatter (tests/warp_motion_ref.py): k_warp_scatter in which
// a hit pixel of a mesh that moved in the interval the last temporal step ended scatters X* = X_s + advance * (X_s - X') for X_s, X'
// where its hit (u, v) was on the triangle's previous vertices (fovpt_post_pixel.h, as k_temporal_motion's).  The common case -- an
// unmarked mesh -- pays for the hit record, one word of the triangle record and the mark; the branch is per lane.
__global__ __launch_bounds__(FOVPT_BLOCK) void k_warp_scatter_motion(const FrameDev fd, const WarpArgs a, const WarpMotionArgs m,
                                                                     const uint32_t* __restrict__ prim, const float4* __restrict__ pos,
                                                                     unsigned long long* __restrict__ keys, unsigned long long* __restrict__ counts)
{
    uint32_t x, y, s;
    bool landed = false;
    if (tile_pixel(fd.w, fd.h, x, y, s)) {                                // (lanes outside the frame go on to count_wave)
        const uint32_t p = prim[s];
        const bool miss = p == 0xffffffffu;
        V3 v;
        if (!miss) {
            V3 X = v3(pos[s]);
            const float4 hit = m.hit[s];
            const uint64_t rec = (uint64_t)__float_as_uint(hit.w) << 4;   // byte offset of the triangle record, as k_gbuffer_fill's
            if (rec + sizeof(TriRec) <= m.tri_bytes && p < m.num_prims) { // (a G-buffer of this frame's trace: always)
                const float4* tr = (const float4*)((const char*)m.tris + rec);
                const uint32_t mesh = __float_as_uint(tr[2].z);
                if (mesh < m.num_meshes && m.mark[mesh] == m.epoch) {
                    V3 A, B, Cc;
                    previous_vertices(m.tri_vidx, m.vtx_prev, p, A, B, Cc);
                    const V3 d = X - previous_point(hit, A, B, Cc);
                    X = X + m.advance * d;
                }
            }
            v = X - v3(a.eye[0], a.eye[1], a.eye[2]);
        } else v = pixel_ray(fd, x, y);                                  // the sky is at infinity: only rotation moves it
        landed = scatter_key(fd, a, v, miss, s, keys);                    // (a non-finite X* does not land)
    }
    count_wave(landed, &count_slot(counts)[0]);
}

// fovpt_warp_depth's scatter (tests/warp_depth_ref.py): k_warp_scatter with the source point rebuilt from a
// depth image.  fd: the size and the camera the depths were rendered with, all that is read of it.  A pixel at depth z along W is
// eye + z * pixel_ray; +inf is the sky, which scatters its direction as a miss does; NaN, <= 0 and -inf scatter nothing.
__global__ __launch_bounds__(FOVPT_BLOCK) void k_warp_scatter_depth(const FrameDev fd, const WarpArgs a, const float* __restrict__ depth,
                                                                    unsigned long long* __restrict__ keys, unsigned long long* __restrict__ counts)
{
    uint32_t x, y, s;
    bool landed = false;
    if (tile_pixel(fd.w, fd.h, x, y, s)) {                                // (lanes outside the frame go on to count_wave)
        const float z = depth[s];
        if (z > 0.0f) {                                                  // (NaN fails)
            const bool miss = z == INFINITY;
            V3 v = pixel_ray(fd, x, y);
            if (!miss) v = (v3(fd.eye[0], fd.eye[1], fd.eye[2]) + z * v) - v3(a.eye[0], a.eye[1], a.eye[2]);
            landed = scatter_key(fd, a, v, miss, s, keys);
        }
    }
    count_wave(landed, &count_slot(counts)[0]);
}

// the largest non-empty key, or 0
__device__ inline unsigned long long farthest(unsigned long long best, unsigned long long k) { return k != WARP_EMPTY && k > best ? k : best; }

// in_color / out_color and in_rgba / out_rgba: both null where the image is not warped; out_map: may be null
__global__ __launch_bounds__(FOVPT_BLOCK) void k_warp_resolve(int w, int h, int radius, const unsigned long long* __restrict__ keys,
                                                              const fovpt_float4* __restrict__ in_color, const uint32_t* __restrict__ in_rgba,
                                                              fovpt_float4* __restrict__ out_color, uint32_t* __restrict__ out_rgba,
                                                              uint32_t* __restrict__ out_map, unsigned long long* __restrict__ counts)
{
    int x, y;
    uint32_t q;
    const bool in = tile_pixel(w, h, x, y, q);
    uint32_t cls = 3u;                                                   // (outside the frame: no class)
    if (in) {
        unsigned long long k = keys[q];
        cls = 0u;
        if (k == WARP_EMPTY) {
            unsigned long long best = 0ull;                              // (no key is 0: a landed depth word is not)
            for (int r = 1; r <= radius && best == 0ull; r++) {
                const int x0 = max(x - r, 0), x1 = min(x + r, w - 1);
                if (y - r >= 0)
                    for (int qx = x0; qx <= x1; qx++) best = farthest(best, keys[(size_t)(y - r) * (size_t)w + (size_t)qx]);
                if (y + r < h)
                    for (int qx = x0; qx <= x1; qx++) best = farthest(best, keys[(size_t)(y + r) * (size_t)w + (size_t)qx]);
                const int y0 = max(y - r + 1, 0), y1 = min(y + r - 1, h - 1);
                if (x - r >= 0)
                    for (int qy = y0; qy <= y1; qy++) best = farthest(best, keys[(size_t)qy * (size_t)w + (size_t)(x - r)]);
                if (x + r < w)
                    for (int qy = y0; qy <= y1; qy++) best = farthest(best, keys[(size_t)qy * (size_t)w + (size_t)(x + r)]);
            }
            cls = best != 0ull ? 1u : 2u;
            k = best;
        }
        const uint32_t src = cls == 2u ? q : (uint32_t)k;                // (a key's low word is a source pixel: below w * h)
        if (out_color) out_color[q] = in_color[src];
        if (out_rgba) out_rgba[q] = in_rgba[src];
        if (out_map) out_map[q] = src | (cls << 30);
    }
    unsigned long long* slot = count_slot(counts);
    count_wave(cls == 0u, &slot[1]);
    count_wave(cls == 1u, &slot[2]);
    count_wave(cls == 2u, &slot[3]);
}

}  // namespace

void fovpt_launch_warp_scatter(hipStream_t st, const FrameDev& fd, const WarpArgs& a, const uint32_t* prim, const float4* pos, uint64_t* keys,
                               uint64_t* counts)
{
    hipLaunchKernelGGL(k_warp_scatter, fovpt_tile_grid(fd.w, fd.h), dim3(FOVPT_BLOCK), 0, st, fd, a, prim, pos, (unsigned long long*)keys,
                       (unsigned long long*)counts);
}

void fovpt_launch_warp_scatter_motion(hipStream_t st, const FrameDev& fd, const WarpArgs& a, const WarpMotionArgs& m, const uint32_t* prim,
                                      const float4* pos, uint64_t* keys, uint64_t* counts)
{
    hipLaunchKernelGGL(k_warp_scatter_motion, fovpt_tile_grid(fd.w, fd.h), dim3(FOVPT_BLOCK), 0, st, fd, a, m, prim, pos,
                       (unsigned long long*)keys, (unsigned long long*)counts);
}

void fovpt_launch_warp_scatter_depth(hipStream_t st, const FrameDev& fd, const WarpArgs& a, const float* depth, uint64_t* keys, uint64_t* counts)
{
    hipLaunchKernelGGL(k_warp_scatter_depth, fovpt_tile_grid(fd.w, fd.h), dim3(FOVPT_BLOCK), 0, st, fd, a, depth, (unsigned long long*)keys,
                       (unsigned long long*)counts);
}

void fovpt_launch_warp_resolve(hipStream_t st, int w, int h, int radius, const uint64_t* keys, const fovpt_float4* in_color, const uint32_t* in_rgba,
                               fovpt_float4* out_color, uint32_t* out_rgba, uint32_t* out_map, uint64_t* counts)
{
    hipLaunchKernelGGL(k_warp_resolve, fovpt_tile_grid(w, h), dim3(FOVPT_BLOCK), 0, st, w, h, radius, (const unsigned long long*)keys, in_color,
                       in_rgba, out_color, out_rgba, out_map, (unsigned long long*)counts);
}
