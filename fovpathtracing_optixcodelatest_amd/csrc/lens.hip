// lens.hip -- fovpt_lens: pre-distortion of a finished frame for a head-mounted display's lens, one radial polynomial per colour
// channel, optionally behind a rotation-only re-aim, resampled with nearest, bilinear or Catmull-Rom taps.
//
//   k_lens<FILTER, MONO>   per destination pixel: its lens radius, the polynomial, per channel the source position (and its
//                          homography H to the rendered camera), the window's taps (fovpt_lens_taps.h) and the filter.  MONO: the
//                          three chroma factors have equal bits, so the channels share one position: one window of 16-byte
//                          loads serves all three.  Otherwise three windows, each reading its own component.
//
// One thread per pixel, 64 x 4 pixel tiles (a wave is 64 pixels of a row), no LDS: a direct gather.  The filter and the lookup
// count are template arguments, so a launch carries no per-tap branch on them.  The definition, operation by operation, is
// tests/lens_ref.py; -ffp-contract=off keeps every product and sum of it a separate binary32 op.
#include "fovpt_device.h"
#include "fovpt_pixel.h"
#include "fovpt_lens_taps.h"

namespace {

// Catmull-Rom weights of the fraction t
__device__ inline void cubic_weights(float t, float* w)
{
    w[0] = ((-0.5f * t + 1.0f) * t - 0.5f) * t;
    w[1] = ((1.5f * t - 2.5f) * t) * t + 1.0f;
    w[2] = ((-1.5f * t + 2.0f) * t + 0.5f) * t;
    w[3] = ((0.5f * t - 0.5f) * t) * t;
}

// Steps 4 to 7 for one chroma factor: the source position and its window.  false: the channel is invalid
template <int FILTER>
__device__ inline bool lens_window(const LensArgs& a, int w, int h, float px, float py, float fc, LensAxis& ax, LensAxis& ay)
{
    float sx = (px * fc) * a.src_scale[0] + a.src_center[0];
    float sy = (py * fc) * a.src_scale[1] + a.src_center[1];
    if (a.reaim) {
        const float hx = (a.H[0] * sx + a.H[1] * sy) + a.H[2];
        const float hy = (a.H[3] * sx + a.H[4] * sy) + a.H[5];
        const float hz = (a.H[6] * sx + a.H[7] * sy) + a.H[8];
        if (!(hz > 0.0f)) return false;
        sx = hx / hz;
        sy = hy / hz;
    }
    const float fx = ((sx + 1.0f) * 0.5f) * (float)w - 0.5f;
    const float fy = ((sy + 1.0f) * 0.5f) * (float)h - 0.5f;
    return lens_taps(fx, fy, w, h, FILTER, ax, ay);
}

// Step 8 over a window.  NC = 3: the three channels of one window from 16-byte loads; NC = 1: channel c0 alone, from its own
// component.  v[k] is channel c0 + k.
template <int FILTER, int NC>
__device__ inline void lens_filter(const LensArgs& a, int w, int h, const fovpt_float4* __restrict__ in, const LensAxis& ax, const LensAxis& ay,
                                   int c0, float* v)
{
    constexpr int N = FILTER == FOVPT_LENS_TAPS_NEAREST ? 1 : FILTER == FOVPT_LENS_TAPS_BILINEAR ? 2 : 4;
    float tap[N][N][NC];
    bool any = false;
#pragma unroll
    for (int j = 0; j < N; j++) {
        const uint32_t qy = lens_tap(ay, j);
        const bool iny = lens_tap_inside(qy, h);
#pragma unroll
        for (int i = 0; i < N; i++) {
            const uint32_t qx = lens_tap(ax, i);
#pragma unroll
            for (int k = 0; k < NC; k++) tap[j][i][k] = a.border[c0 + k];
            if (iny && lens_tap_inside(qx, w)) {
                any = true;
                const uint32_t q = qy * (uint32_t)w + qx;                  // (inside the frame: below w * h < 2^31)
                if constexpr (NC == 3) {
                    const fovpt_float4 t = in[q];
                    tap[j][i][0] = t.x; tap[j][i][1] = t.y; tap[j][i][2] = t.z;
                } else {
                    tap[j][i][0] = (&in[q].x)[c0];
                }
            }
        }
    }
    if constexpr (FILTER == FOVPT_LENS_TAPS_NEAREST) {
#pragma unroll
        for (int k = 0; k < NC; k++) v[k] = tap[0][0][k];
    } else if constexpr (FILTER == FOVPT_LENS_TAPS_BILINEAR) {
        const float tx = ax.t, ty = ay.t;
#pragma unroll
        for (int k = 0; k < NC; k++) {
            const float top = (1.0f - tx) * tap[0][0][k] + tx * tap[0][1][k];
            const float bottom = (1.0f - tx) * tap[1][0][k] + tx * tap[1][1][k];
            v[k] = (1.0f - ty) * top + ty * bottom;
        }
    } else {
        float wx[4], wy[4];
        cubic_weights(ax.t, wx);
        cubic_weights(ay.t, wy);
#pragma unroll
        for (int k = 0; k < NC; k++) {
            float row[4];
#pragma unroll
            for (int j = 0; j < 4; j++) row[j] = ((wx[0] * tap[j][0][k] + wx[1] * tap[j][1][k]) + wx[2] * tap[j][2][k]) + wx[3] * tap[j][3][k];
            const float s = ((wy[0] * row[0] + wy[1] * row[1]) + wy[2] * row[2]) + wy[3] * row[3];
            v[k] = s < 0.0f ? 0.0f : s;
        }
    }
    if (!any) {                                                            // a window with no tap inside the frame: the border, exactly
#pragma unroll
        for (int k = 0; k < NC; k++) v[k] = a.border[c0 + k];
    }
}

template <int FILTER, bool MONO>
__global__ __launch_bounds__(FOVPT_BLOCK) void k_lens(int w, int h, const LensArgs a, const fovpt_float4* __restrict__ in,
                                                      fovpt_float4* __restrict__ out_color, uint32_t* __restrict__ out_rgba)
{
    uint32_t x, y, p;
    if (!tile_pixel(w, h, x, y, p)) return;
    const float nx = (float)(2u * x + 1u) / (float)w - 1.0f;
    const float ny = (float)(2u * y + 1u) / (float)h - 1.0f;
    const float px = (nx - a.center[0]) * a.scale[0];
    const float py = (ny - a.center[1]) * a.scale[1];
    const float r2 = px * px + py * py;
    float o[4] = {a.border[0], a.border[1], a.border[2], a.border[3]};
    if (r2 <= a.clip_r2) {
        const float f = a.k[0] + r2 * (a.k[1] + r2 * (a.k[2] + r2 * a.k[3]));
        LensAxis ax, ay;
        if (MONO) {
            if (lens_window<FILTER>(a, w, h, px, py, f * a.chroma[0], ax, ay)) lens_filter<FILTER, 3>(a, w, h, in, ax, ay, 0, o);
        } else {
#pragma unroll
            for (int c = 0; c < 3; c++)
                if (lens_window<FILTER>(a, w, h, px, py, f * a.chroma[c], ax, ay)) lens_filter<FILTER, 1>(a, w, h, in, ax, ay, c, &o[c]);
        }
        o[3] = 1.0f;
    }
    out_color[p] = fovpt_float4{o[0], o[1], o[2], o[3]};
    const V3 c = v3(o[0], o[1], o[2]);
    out_rgba[p] = a.encode == FOVPT_LENS_ENCODE_RESOLVE ? resolved_rgba(c) : make_color(c);   // (o[3] is the border's or 1: not store_resolved)
}

template <int FILTER>
void launch(hipStream_t st, int w, int h, const LensArgs& a, const fovpt_float4* in, fovpt_float4* out_color, uint32_t* out_rgba)
{
    const dim3 grid = fovpt_tile_grid(w, h);
    if (a.mono) hipLaunchKernelGGL((k_lens<FILTER, true>), grid, dim3(FOVPT_BLOCK), 0, st, w, h, a, in, out_color, out_rgba);
    else hipLaunchKernelGGL((k_lens<FILTER, false>), grid, dim3(FOVPT_BLOCK), 0, st, w, h, a, in, out_color, out_rgba);
}

}  // namespace

// in is neither output (a pixel reads other pixels'); a.filter and a.encode are checked by the caller
void fovpt_launch_lens(hipStream_t st, int w, int h, const LensArgs& a, const fovpt_float4* in, fovpt_float4* out_color, uint32_t* out_rgba)
{
    if (a.filter == FOVPT_LENS_NEAREST) launch<FOVPT_LENS_TAPS_NEAREST>(st, w, h, a, in, out_color, out_rgba);
    else if (a.filter == FOVPT_LENS_BILINEAR) launch<FOVPT_LENS_TAPS_BILINEAR>(st, w, h, a, in, out_color, out_rgba);
    else launch<FOVPT_LENS_TAPS_BICUBIC>(st, w, h, a, in, out_color, out_rgba);
}
