// bloom.hip -- fovpt_bloom: HDR glare ahead of the tone map.
//
//   k_bloom_prefilter   bright pass and first downsample: one thread per texel of level 0, a block a 64 x 4 tile of them, so that
//                       a wave's two source rows are each one contiguous 2 KiB read.  GAINS: the gain of each of the four source
//                       pixels by the fill of its last writer (the search exists in that instantiation only).  The constants of
//                       step 0 are computed here in fp32, from cfg.exposure or from fovpt_expose's device record
//   k_bloom_down        level k from level k - 1: the 4 x 4 binomial taps, one thread per destination texel
//   k_bloom_up          u_k = d_k + spread * up(u_{k+1}), in place over d_k, one thread per texel of level k
//   k_bloom_composite   per pixel: out = in + intensity * up(u_0), and the rgba8 of every stage
//
// The definition, operation by operation, is tests/bloom_ref.py; -ffp-contract=off keeps every product and sum of it a separate
// binary32 op.  The pyramid's fourth channel is 0 everywhere.
#include "fovpt_device.h"
#include "fovpt_pixel.h"
#include "fovpt_stream.h"           // st_stream: the composite's outputs are written once and read by a later stage

namespace {

#define BLOOM_TX 64                     // a block is a BLOOM_TX x BLOOM_TY tile of destination texels (pixels for the composite)
#define BLOOM_TY 4
#ifndef FOVPT_BLOOM_OUT
#define FOVPT_BLOOM_OUT 4               // the composite's stores, a knob of fovpt_stream.h: 0 plain, 4 nt (measured no worse: DESIGN.md, section 34)
#endif
static_assert(BLOOM_TX == FOVPT_WAVE, "a wave per tile row");

__device__ inline float fmin2(float a, float b) { return a < b ? a : b; }      // the definition's min and max
__device__ inline float fmax2(float a, float b) { return a > b ? a : b; }
__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// the tile and texel of a thread in a grid of tiles over a W x H level; false: outside the level
__device__ inline bool tile_texel(int W, int H, int& X, int& Y)
{
    const uint32_t tiles_x = ((uint32_t)W + BLOOM_TX - 1) / BLOOM_TX;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    X = (int)(tx * BLOOM_TX + threadIdx.x);
    Y = (int)(ty * BLOOM_TY + threadIdx.y);
    return X < W && Y < H;
}

// step 2 of the definition: texel (X, Y) of the level below S (Ws x Hs)
__device__ inline float4 down_texel(const float4* S, int Ws, int Hs, int X, int Y)
{
    float ar = 0.0f, ag = 0.0f, ab = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int sy = clampi(2 * Y - 1 + j, 0, Hs - 1);
        const int bj = (j == 0 || j == 3) ? 1 : 3;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int sx = clampi(2 * X - 1 + i, 0, Ws - 1);
            const int bi = (i == 0 || i == 3) ? 1 : 3;
            const float wgt = (float)(bj * bi) * 0.015625f;
            const float4 s = S[(size_t)sy * (size_t)Ws + (size_t)sx];
            ar = ar + wgt * s.x; ag = ag + wgt * s.y; ab = ab + wgt * s.z;
        }
    }
    return make_float4(ar, ag, ab, 0.0f);
}

// step 3: the level S (Ws x Hs) seen from (x, y) of a grid twice as fine
__device__ inline V3 up_texel(const float4* S, int Ws, int Hs, int x, int y)
{
    const int ax = x >> 1, ay = y >> 1;
    const int bx = clampi((x & 1) ? ax + 1 : ax - 1, 0, Ws - 1), by = clampi((y & 1) ? ay + 1 : ay - 1, 0, Hs - 1);
    const float4 s00 = S[(size_t)ay * (size_t)Ws + (size_t)ax], s10 = S[(size_t)ay * (size_t)Ws + (size_t)bx];
    const float4 s01 = S[(size_t)by * (size_t)Ws + (size_t)ax], s11 = S[(size_t)by * (size_t)Ws + (size_t)bx];
    const V3 r0 = v3(0.75f * s00.x + 0.25f * s10.x, 0.75f * s00.y + 0.25f * s10.y, 0.75f * s00.z + 0.25f * s10.z);
    const V3 r1 = v3(0.75f * s01.x + 0.25f * s11.x, 0.75f * s01.y + 0.25f * s11.y, 0.75f * s01.z + 0.25f * s11.z);
    return v3(0.75f * r0.x + 0.25f * r1.x, 0.75f * r0.y + 0.25f * r1.y, 0.75f * r0.z + 0.25f * r1.z);
}

// step 4 for one texel: d + spread * up
__device__ inline float4 combine(const float4& d, float spread, const V3& u)
{
    return make_float4(d.x + spread * u.x, d.y + spread * u.y, d.z + spread * u.z, 0.0f);
}

template <bool GAINS>
__global__ __launch_bounds__(BLOOM_TX * BLOOM_TY) void k_bloom_prefilter(const FrameDev fd, const BloomArgs a, const ExposeState* __restrict__ state,
                                                                          const float4* __restrict__ in, float4* __restrict__ d0)
{
    const int w = fd.w, h = fd.h, W0 = (w + 1) >> 1, H0 = (h + 1) >> 1;
    int X, Y;
    if (!tile_texel(W0, H0, X, Y)) return;
    // step 0 (every thread the same values)
    const float E = (state && state->steps != 0ull) ? state->exposure : a.exposure;
    const float T = a.threshold / E, K = a.knee / E, K2 = 2.0f * K, K4 = 4.0f * K, TK = T - K;
    const bool karis = (a.flags & FOVPT_BLOOM_KARIS) != 0;
    float4 c[4];
#pragma unroll
    for (int j = 0; j < 2; j++) {                                     // the loads first: four in flight
        const int py = min(2 * Y + j, h - 1);
#pragma unroll
        for (int i = 0; i < 2; i++) c[2 * j + i] = in[(size_t)py * (size_t)w + (size_t)min(2 * X + i, w - 1)];
    }
    float nr = 0.0f, ng = 0.0f, nb = 0.0f, den = 0.0f;
#pragma unroll
    for (int j = 0; j < 2; j++) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const float4 p = c[2 * j + i];
            const float L = luma(p.x, p.y, p.z);
            const float s = fmax2(0.0f, fmin2(L - TK, K2));
            const float q = K > 0.0f ? (s * s) / K4 : 0.0f;
            const float m = fmax2(fmax2(q, L - T), 0.0f) / fmax2(L, 1e-6f);
            const float kw = karis ? 1.0f / (1.0f + L) : 1.0f;
            float g = 1.0f;
            if (GAINS) {
                int wp = 0;
                uint32_t wlx, wly;
                if (!find_last_writer(fd, (uint32_t)min(2 * X + i, w - 1), (uint32_t)min(2 * Y + j, h - 1), wp, wlx, wly)) g = 0.0f;
                else g = by_level(a.gain, a.uniform, fd.pass[wp].fill);
            }
            const float wt = g * kw;
            nr = nr + wt * (p.x * m); ng = ng + wt * (p.y * m); nb = nb + wt * (p.z * m);
            den = den + kw;
        }
    }
    d0[(size_t)Y * (size_t)W0 + (size_t)X] = make_float4(nr / den, ng / den, nb / den, 0.0f);
}

// src: level k - 1 (Ws x Hs); dst: level k
__global__ __launch_bounds__(BLOOM_TX * BLOOM_TY) void k_bloom_down(const float4* __restrict__ src, int Ws, int Hs, float4* __restrict__ dst)
{
    const int W = (Ws + 1) >> 1, H = (Hs + 1) >> 1;
    int X, Y;
    if (!tile_texel(W, H, X, Y)) return;
    dst[(size_t)Y * (size_t)W + (size_t)X] = down_texel(src, Ws, Hs, X, Y);
}

// lvl: d_k (W x H), overwritten by u_k; below: u_{k+1} (Ws x Hs)
__global__ __launch_bounds__(BLOOM_TX * BLOOM_TY) void k_bloom_up(float4* __restrict__ lvl, int W, int H, const float4* __restrict__ below, int Ws, int Hs,
                                                                   float spread)
{
    int x, y;
    if (!tile_texel(W, H, x, y)) return;
    const size_t idx = (size_t)y * (size_t)W + (size_t)x;
    lvl[idx] = combine(lvl[idx], spread, up_texel(below, Ws, Hs, x, y));
}

// `in` and `out_color` may be the same buffer: a thread reads only its own pixel of `in`, before it writes out_color
__global__ __launch_bounds__(BLOOM_TX * BLOOM_TY) void k_bloom_composite(int w, int h, float intensity, const float4* __restrict__ u0, const float4* in,
                                                                          float4* out_color, uint32_t* __restrict__ out_rgba)
{
    int x, y;
    if (!tile_texel(w, h, x, y)) return;
    const size_t idx = (size_t)y * (size_t)w + (size_t)x;
    const float4 c = in[idx];
    const V3 B = up_texel(u0, (w + 1) >> 1, (h + 1) >> 1, x, y);
    const V3 o = v3(c.x + intensity * B.x, c.y + intensity * B.y, c.z + intensity * B.z);
    st_stream<FOVPT_BLOOM_OUT>(&out_color[idx], make_float4(o.x, o.y, o.z, c.w));
    st_stream<FOVPT_BLOOM_OUT>(&out_rgba[idx], resolved_rgba(o));      // (c.w kept and streaming stores: not store_resolved)
}

dim3 tile_grid(int W, int H)
{
    return dim3((uint32_t)(((size_t)W + BLOOM_TX - 1) / BLOOM_TX * (((size_t)H + BLOOM_TY - 1) / BLOOM_TY)));
}

}  // namespace

void fovpt_bloom_level(int w, int h, int k, int* W, int* H, size_t* first)
{
    size_t off = 0;
    int lw = (w + 1) / 2, lh = (h + 1) / 2;
    for (int j = 0; j < k; j++) { off += (size_t)lw * (size_t)lh; lw = (lw + 1) / 2; lh = (lh + 1) / 2; }
    *W = lw; *H = lh; *first = off;
}

void fovpt_launch_bloom(hipStream_t st, const FrameDev& fd, const BloomArgs& a, int levels, const ExposeState* state, const fovpt_float4* in,
                        float4* pyramid, fovpt_float4* out_color, uint32_t* out_rgba)
{
    const dim3 block(BLOOM_TX, BLOOM_TY);
    const int w = fd.w, h = fd.h;
    int W[FOVPT_BLOOM_MAX_LEVELS], H[FOVPT_BLOOM_MAX_LEVELS];
    size_t first[FOVPT_BLOOM_MAX_LEVELS];
    for (int k = 0; k < levels; k++) fovpt_bloom_level(w, h, k, &W[k], &H[k], &first[k]);
    if (a.flags & FOVPT_BLOOM_GAINS) hipLaunchKernelGGL(k_bloom_prefilter<true>, tile_grid(W[0], H[0]), block, 0, st, fd, a, state, (const float4*)in, pyramid);
    else hipLaunchKernelGGL(k_bloom_prefilter<false>, tile_grid(W[0], H[0]), block, 0, st, fd, a, state, (const float4*)in, pyramid);
    // one launch per level down and back (one workgroup making the small levels in LDS measured slower: EXPERIMENTS.md)
    for (int k = 1; k < levels; k++)
        hipLaunchKernelGGL(k_bloom_down, tile_grid(W[k], H[k]), block, 0, st, (const float4*)(pyramid + first[k - 1]), W[k - 1], H[k - 1], pyramid + first[k]);
    for (int k = levels - 2; k >= 0; k--)
        hipLaunchKernelGGL(k_bloom_up, tile_grid(W[k], H[k]), block, 0, st, pyramid + first[k], W[k], H[k], (const float4*)(pyramid + first[k + 1]), W[k + 1],
                           H[k + 1], a.spread);
    hipLaunchKernelGGL(k_bloom_composite, tile_grid(w, h), block, 0, st, w, h, a.intensity, (const float4*)pyramid, (const float4*)in, (float4*)out_color,
                       out_rgba);
}
