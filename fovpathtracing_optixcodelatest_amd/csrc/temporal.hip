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
#include "fovpt_post_pixel.h"

namespace {

// `in` and `out_color` may be the same buffer: a thread reads only its own pixel of `in`, before it writes out_color
__global__ __launch_bounds__(FOVPT_BLOCK) void k_temporal(const FrameDev fd, TemporalArgs a, const fovpt_float4* in, GBufferDev g, GBufferDev gp,
                                                          const float4* __restrict__ hist_prev, float4* __restrict__ hist_out,
                                                          fovpt_float4* out_color, uint32_t* __restrict__ out_rgba)
{
    uint32_t x, y, idx;
    if (!tile_pixel(fd.w, fd.h, x, y, idx)) return;
    const fovpt_float4 c = in[idx];
    int wp = 0;
    uint32_t wlx, wly;
    const int cap = history_cap(fd, a, find_last_writer(fd, x, y, wp, wlx, wly), wp);
    float nh = 0.0f;
    V3 H = v3(0.0f);
    temporal_history(fd, a, GLazy{g, idx}, gp, hist_prev, x, y, cap, H, nh);          // (fovpt_post_pixel.h)
    temporal_blend(c, H, nh, cap, idx, hist_out, out_color, out_rgba);
}

// k_temporal with a moving surface's point and normal taken where the surface was at the previous step
// (temporal_motion_history, fovpt_post_pixel.h; tests/temporal_motion_ref.py).  With m.out_motion (px - x, py - y, a.z, 1) is
// stored, (0, 0, 0, 0) where the pixel does not reproject.
__global__ __launch_bounds__(FOVPT_BLOCK) void k_temporal_motion(const FrameDev fd, TemporalArgs a, TemporalMotionArgs m, const fovpt_float4* in,
                                                                 GBufferDev g, GBufferDev gp, const float4* __restrict__ hist_prev,
                                                                 float4* __restrict__ hist_out, fovpt_float4* out_color,
                                                                 uint32_t* __restrict__ out_rgba)
{
    uint32_t x, y, idx;
    if (!tile_pixel(fd.w, fd.h, x, y, idx)) return;
    const fovpt_float4 c = in[idx];
    int wp = 0;
    uint32_t wlx, wly;
    const int cap = history_cap(fd, a, find_last_writer(fd, x, y, wp, wlx, wly), wp);
    const bool want_motion = m.out_motion != nullptr;                      // (wave-uniform: a kernel argument)
    float nh = 0.0f;
    V3 H = v3(0.0f);
    float4 mv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    temporal_motion_history(fd, a, m, GLazy{g, idx}, gp, hist_prev, x, y, idx, cap, want_motion, H, nh, mv);
    if (want_motion) m.out_motion[idx] = fovpt_float4{mv.x, mv.y, mv.z, mv.w};
    temporal_blend(c, H, nh, cap, idx, hist_out, out_color, out_rgba);
}

}  // namespace

void fovpt_launch_temporal_motion(hipStream_t st, const FrameDev& fd, const TemporalArgs& a, const TemporalMotionArgs& m, const fovpt_float4* in,
                                  GBufferDev g, GBufferDev gp, const float4* hist_prev, float4* hist_out, fovpt_float4* out_color,
                                  uint32_t* out_rgba)
{
    hipLaunchKernelGGL(k_temporal_motion, fovpt_tile_grid(fd.w, fd.h), dim3(FOVPT_BLOCK), 0, st, fd, a, m, in, g, gp, hist_prev, hist_out,
                       out_color, out_rgba);
}

void fovpt_launch_temporal(hipStream_t st, const FrameDev& fd, const TemporalArgs& a, const fovpt_float4* in, GBufferDev g, GBufferDev gp,
                           const float4* hist_prev, float4* hist_out, fovpt_float4* out_color, uint32_t* out_rgba)
{
    hipLaunchKernelGGL(k_temporal, fovpt_tile_grid(fd.w, fd.h), dim3(FOVPT_BLOCK), 0, st, fd, a, in, g, gp, hist_prev, hist_out, out_color, out_rgba);
}
