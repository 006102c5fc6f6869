// post_fused.hip -- fovpt_post with the reconstruction and the temporal step both on: one kernel for the two.
//
//   k_reconstruct_temporal<motion>   per pixel k_reconstruct's body, its colour kept in registers, then k_temporal's
//                (motion false) or k_temporal_motion's (true) body with that colour as the step's input.  k_temporal reads only
//                its own pixel of its input and k_reconstruct writes exactly that pixel, so the result is the two kernels' bit
//                for bit, without the 16 B store and load between them, with one last-writer search and one read of the
//                pixel's own G-buffer entry.
//
// One thread per pixel, 64 x 4 pixel tiles, no LDS.  The bodies are those of fovpt_post_pixel.h; -ffp-contract=off keeps
// every product and sum a separate binary32 op.
#include "fovpt_device.h"
#include "fovpt_pixel.h"
#include "fovpt_post_pixel.h"

namespace {

// `in` and `albedo` are read at neighbouring pixels: no output may be one of them (fovpt_post checks)
template <bool MOTION>
__global__ __launch_bounds__(FOVPT_BLOCK) void k_reconstruct_temporal(const FrameDev fd, ReconstructArgs ra, TemporalArgs ta, TemporalMotionArgs m,
                                                                      const fovpt_float4* __restrict__ in, const fovpt_float4* __restrict__ albedo,
                                                                      GBufferDev g, GBufferDev gp, const float4* __restrict__ hist_prev,
                                                                      float4* __restrict__ hist_out, fovpt_float4* __restrict__ out_color,
                                                                      uint32_t* __restrict__ out_rgba)
{
    uint32_t x, y, idx;
    if (!tile_pixel(fd.w, fd.h, x, y, idx)) return;
    int wp = 0;
    uint32_t wlx, wly;
    const bool found = find_last_writer(fd, x, y, wp, wlx, wly);           // the reconstruction's level and anchor, the step's cap
    const int cap = history_cap(fd, ta, found, wp);
    const bool rec = found && reconstruct_level_on(ra, fd.pass[wp].fill);
    const bool want_motion = MOTION && m.out_motion != nullptr;            // (wave-uniform: a kernel argument)
    GRegs own = {0xffffffffu, make_float4(0.f, 0.f, 0.f, -1.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    if (rec || (ta.reproject && (cap > 1 || want_motion))) {               // what either body reads of the pixel's own entry
        own.prim_ = g.prim[idx]; own.pos_ = g.pos[idx]; own.nrm_ = g.nrm[idx];
    }
    V3 o;
    const bool done = rec && reconstruct_pixel(fd, ra, in, albedo, g, own, x, y, idx, wp, wlx, wly, o);
    const fovpt_float4 c = done ? fovpt_float4{o.x, o.y, o.z, 1.0f} : in[idx];   // (read here: not held across the reconstruction)
    float nh = 0.0f;
    V3 H = v3(0.0f);
    if (MOTION) {
        float4 mv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        temporal_motion_history(fd, ta, m, own, gp, hist_prev, x, y, idx, cap, want_motion, H, nh, mv);
        if (want_motion) m.out_motion[idx] = fovpt_float4{mv.x, mv.y, mv.z, mv.w};
    } else temporal_history(fd, ta, own, gp, hist_prev, x, y, cap, H, nh);
    temporal_blend(c, H, nh, cap, idx, hist_out, out_color, out_rgba);
}

}  // namespace

void fovpt_launch_reconstruct_temporal(hipStream_t st, const FrameDev& fd, const ReconstructArgs& ra, const TemporalArgs& ta,
                                       const TemporalMotionArgs* m, const fovpt_float4* in, const fovpt_float4* albedo, GBufferDev g,
                                       GBufferDev gp, const float4* hist_prev, float4* hist_out, fovpt_float4* out_color, uint32_t* out_rgba)
{
    const dim3 grid = fovpt_tile_grid(fd.w, fd.h);
    if (m) hipLaunchKernelGGL(k_reconstruct_temporal<true>, grid, dim3(FOVPT_BLOCK), 0, st, fd, ra, ta, *m, in, albedo, g, gp, hist_prev, hist_out,
                              out_color, out_rgba);
    else {
        TemporalMotionArgs none = {};
        hipLaunchKernelGGL(k_reconstruct_temporal<false>, grid, dim3(FOVPT_BLOCK), 0, st, fd, ra, ta, none, in, albedo, g, gp, hist_prev, hist_out,
                           out_color, out_rgba);
    }
}
