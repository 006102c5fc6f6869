// focus.hip -- fovpt_focus: gaze-metered focus distance and depth of field.
//
//   k_focus_meter    one block over the gaze disc's bounding square, clipped to the frame (at most 129 x 129 pixels): the histogram
//                    of the hit distance t of the disc's pixels in LDS (fovpt_expose's bins from the bits of t, integer sums: any
//                    order, same result, no global atomics), a scan, the bin of the asked rank, the adapt step in reciprocal
//                    distance, into the device state record
//   k_focus_radius   per pixel: the blur radius r from |1 / t - 1 / focus| (the focus read from the state record, or an argument:
//                    FOCUS_FIXED) and tp = t, +inf on a miss, as one 8-byte pair; out_coc if asked
//   k_focus_gather   per pixel: the weighted mean of the taps that cover it.  A block makes 32 x 16 outputs, a thread each, from its
//                    tile and an apron of max_radius pixels staged in LDS: (radius, tp), what decides whether a tap covers, as
//                    one 8-byte entry read by every lane with one ds_read_b64 per tap, and the colour as a 16-byte entry beside
//                    it, read by the lanes the tap covers alone.  A row of the image is a row of consecutive entries: the lanes
//                    of a wave's half are 32 neighbours of one row and every tap moves them by the same offset, so a lane group
//                    always reads consecutive addresses and no read conflicts, whatever the row stride.  Non-covering taps add
//                    nothing, so with m the largest radius of the tile and its apron the loops run to
//                    min(max_radius, floor(m + 0.5f)) -- the sum in fp32, as a tap's own e = re + 0.5f -- and a tile where
//                    that is 0 is a copy (tests/test_focus_cpu.py checks both against the full loops)
//
// The definition, operation by operation, is tests/focus_ref.py; -ffp-contract=off keeps every product and sum of it a separate
// binary32 op.
#include "fovpt_device.h"
#include "fovpt_pixel.h"

namespace {

#define FOCUS_BINS FOVPT_FOCUS_BINS
#define FOCUS_UNROLL 4                  // pixels a thread of the meter has in flight
#define FOCUS_TW FOVPT_FOCUS_TILE_W
#define FOCUS_TH FOVPT_FOCUS_TILE_H
#define FOCUS_LW (FOCUS_TW + 2 * FOVPT_FOCUS_MAX_RADIUS)    // the staged image at the largest apron
#define FOCUS_LH (FOCUS_TH + 2 * FOVPT_FOCUS_MAX_RADIUS)
static_assert(FOCUS_BINS <= FOVPT_FOCUS_BLOCK, "a thread per bin");
static_assert(FOCUS_TW * FOCUS_TH % FOVPT_WAVE == 0 && FOCUS_TW <= FOVPT_WAVE && FOVPT_WAVE % FOCUS_TW == 0, "whole rows in a wave");

// prim / pos: the G-buffer; every index below is of a pixel inside the frame (a's square is clipped on the host)
__global__ __launch_bounds__(FOVPT_FOCUS_BLOCK) void k_focus_meter(int w, const FocusArgs a, const uint32_t* __restrict__ prim,
                                                                   const float4* __restrict__ pos, FocusState* __restrict__ state)
{
    __shared__ uint32_t h[FOCUS_BINS];
    __shared__ uint32_t cum[2][FOCUS_BINS];
    __shared__ int sel;
    const uint32_t k = threadIdx.x;
    if (k < FOCUS_BINS) h[k] = 0u;
    if (k == 0) sel = 0;
    __syncthreads();
    const int bw = a.x1 - a.x0 + 1, bh = a.y1 - a.y0 + 1;               // (either <= 0: nothing to meter)
    const uint32_t n = bw > 0 && bh > 0 ? (uint32_t)bw * (uint32_t)bh : 0u;
    const long long r2 = (long long)a.meter_radius * (long long)a.meter_radius;
    for (uint32_t i0 = k; i0 < n; i0 += FOCUS_UNROLL * FOVPT_FOCUS_BLOCK) {
        float t[FOCUS_UNROLL];
#pragma unroll
        for (int j = 0; j < FOCUS_UNROLL; j++) {                        // the loads first: FOCUS_UNROLL of them in flight
            const uint32_t i = i0 + (uint32_t)j * FOVPT_FOCUS_BLOCK;
            t[j] = 0.0f;
            if (i < n) {
                const uint32_t by = i / (uint32_t)bw, bx = i - by * (uint32_t)bw;
                const long long x = (long long)a.x0 + bx, y = (long long)a.y0 + by;
                const long long dx = x - a.cx, dy = y - a.cy;
                const size_t idx = (size_t)y * (size_t)w + (size_t)x;
                if (dx * dx + dy * dy <= r2 && prim[idx] != 0xffffffffu) t[j] = pos[idx].w;
            }
        }
#pragma unroll
        for (int j = 0; j < FOCUS_UNROLL; j++) {
            if (!(t[j] > 0.0f)) continue;                               // (+inf counts; NaN, 0 and negatives do not)
            const int bin = min(max((int)(__float_as_uint(t[j]) >> 20) - 888, 0), FOCUS_BINS - 1);
            atomicAdd(&h[bin], 1u);
        }
    }
    __syncthreads();
    const bool own = k < FOCUS_BINS;                                     // thread k < 256 owns bin k
    if (own) cum[0][k] = h[k];
    int cur = 0;
    __syncthreads();
    for (uint32_t d = 1; d < FOCUS_BINS; d <<= 1) {                      // inclusive scan (Hillis-Steele, two buffers)
        if (own) cum[cur ^ 1][k] = cum[cur][k] + (k >= d ? cum[cur][k - d] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    const uint32_t T = cum[cur][FOCUS_BINS - 1];
    if (own && T != 0u) {
        const uint32_t rank = (uint32_t)(((unsigned long long)T * (unsigned long long)a.rank_permille) / 1000ull);
        const uint32_t kk = rank < T - 1u ? rank : T - 1u;
        const uint32_t hi = cum[cur][k], lo = hi - h[k];
        if (hi > kk && lo <= kk) sel = (int)k;                           // the smallest bin whose running sum exceeds kk: one thread
    }
    __syncthreads();
    if (k != 0) return;
    const bool first = state->steps == 0ull;
    float D = state->inv_focus, metered, Dm;
    if (T != 0u) {
        metered = __uint_as_float((((uint32_t)sel + 888u) << 20) | 0x80000u);
        Dm = 1.0f / metered;
    } else if (first) {
        metered = a.focus_default;
        Dm = 1.0f / metered;
    } else {
        metered = state->focus;                                         // nothing to meter: the present focus, D stays
        Dm = D;
    }
    if (first) D = Dm;
    else {
        const float rate = Dm > D ? a.adapt_nearer : a.adapt_farther;
        D = D + rate * (Dm - D);
    }
    state->focus_metered = metered;
    state->inv_focus = D;
    state->focus = 1.0f / D;
    state->_pad = 0.0f;
    state->count = (uint64_t)T;
    state->steps = state->steps + 1ull;
}

__global__ __launch_bounds__(FOVPT_BLOCK) void k_focus_radius(uint32_t npix, const FocusArgs a, const FocusState* __restrict__ state,
                                                              const uint32_t* __restrict__ prim, const float4* __restrict__ pos,
                                                              float2* __restrict__ rt, float* __restrict__ out_coc)
{
    const uint32_t idx = blockIdx.x * FOVPT_BLOCK + threadIdx.x;
    if (idx >= npix) return;
    const float D = state ? state->inv_focus : a.inv_focus;
    const bool hit = prim[idx] != 0xffffffffu;
    const float t = pos[idx].w;
    const float i = hit ? 1.0f / t : 0.0f;
    const float s = a.strength * fabsf(i - D), cap = (float)a.max_radius;
    const float r = s < cap ? s : cap;                                   // (a NaN goes to the cap)
    rt[idx] = make_float2(r, hit ? t : __uint_as_float(0x7f800000u));
    if (out_coc) out_coc[idx] = r;
}

// R: max_radius (0 .. FOVPT_FOCUS_MAX_RADIUS), the apron.  in / rt are read across pixels: neither is an output
__global__ __launch_bounds__(FOCUS_TW * FOCUS_TH) void k_focus_gather(int w, int h, int R, const fovpt_float4* __restrict__ in,
                                                                       const float2* __restrict__ rt, fovpt_float4* __restrict__ out_color,
                                                                       uint32_t* __restrict__ out_rgba)
{
    __shared__ float2 s_rt[FOCUS_LH][FOCUS_LW];                          // radius (-1 outside the frame: such a tap never covers), tp
    __shared__ float4 s_c[FOCUS_LH][FOCUS_LW];                           // r, g, b: read only by the lanes the tap covers
    __shared__ uint32_t s_m;                                             // the bits of the largest radius staged (radii are >= 0)
    const int lx = (int)threadIdx.x, ly = (int)threadIdx.y;
    const int x = (int)blockIdx.x * FOCUS_TW + lx, y = (int)blockIdx.y * FOCUS_TH + ly;
    const int gx0 = (int)blockIdx.x * FOCUS_TW - R, gy0 = (int)blockIdx.y * FOCUS_TH - R;
    if (lx == 0 && ly == 0) s_m = 0u;
    __syncthreads();
    float m = 0.0f;
    for (int row = ly; row < FOCUS_TH + 2 * R; row += FOCUS_TH) {
        const int gy = gy0 + row;
        for (int col = lx; col < FOCUS_TW + 2 * R; col += FOCUS_TW) {
            const int gx = gx0 + col;
            float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float2 p = make_float2(-1.0f, 0.0f);
            if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
                const size_t q = (size_t)gy * (size_t)w + (size_t)gx;
                const fovpt_float4 cq = in[q];
                p = rt[q];
                c = make_float4(cq.x, cq.y, cq.z, 0.0f);
                m = p.x > m ? p.x : m;
            }
            s_rt[row][col] = p;
            s_c[row][col] = c;
        }
    }
#pragma unroll
    for (int d = FOVPT_WAVE / 2; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    if (((ly * FOCUS_TW + lx) & (FOVPT_WAVE - 1)) == 0) atomicMax(&s_m, __float_as_uint(m));
    __syncthreads();
    if (x >= w || y >= h) return;                                        // (no barrier below)
    const uint32_t idx = (uint32_t)y * (uint32_t)w + (uint32_t)x;
    const fovpt_float4 own = in[idx];
    const int reach = (int)floorf(__uint_as_float(s_m) + 0.5f);         // no tap further than this along an axis covers any pixel of the tile
    const int B = reach < R ? reach : R;
    V3 o = v3(own.x, own.y, own.z);
    float ow = own.w;
    if (B > 0) {
        const float rp = s_rt[ly + R][lx + R].x, tp = s_rt[ly + R][lx + R].y;
        float den = 0.0f, nr = 0.0f, ng = 0.0f, nb = 0.0f;
        int covering = 0;
        for (int dy = -B; dy <= B; dy++) {
            for (int dx = -B; dx <= B; dx++) {
                const float2 k = s_rt[ly + R + dy][lx + R + dx];         // (rq, tq)
                const float re = k.y > tp ? (k.x < rp ? k.x : rp) : k.x;
                const float e = re + 0.5f, e2 = e * e;
                if ((float)(dx * dx + dy * dy) <= e2) {
                    const float4 q = s_c[ly + R + dy][lx + R + dx];
                    const float g = 1.0f / e2;
                    den = den + g;
                    nr = nr + g * q.x; ng = ng + g * q.y; nb = nb + g * q.z;
                    covering++;
                }
            }
        }
        if (covering > 1) o = v3(nr / den, ng / den, nb / den);
    }
    out_color[idx] = fovpt_float4{o.x, o.y, o.z, ow};
    out_rgba[idx] = resolved_rgba(o);                                    // (the pixel keeps its own w: not store_resolved)
}

}  // namespace

void fovpt_launch_focus_meter(hipStream_t st, int w, const FocusArgs& a, const uint32_t* prim, const float4* pos, FocusState* state)
{
    hipLaunchKernelGGL(k_focus_meter, dim3(1), dim3(FOVPT_FOCUS_BLOCK), 0, st, w, a, prim, pos, state);
}

void fovpt_launch_focus_radius(hipStream_t st, size_t npix, const FocusArgs& a, const FocusState* state, const uint32_t* prim, const float4* pos,
                               float2* rt, float* out_coc)
{
    const dim3 grid((uint32_t)((npix + FOVPT_BLOCK - 1) / FOVPT_BLOCK));
    hipLaunchKernelGGL(k_focus_radius, grid, dim3(FOVPT_BLOCK), 0, st, (uint32_t)npix, a, state, prim, pos, rt, out_coc);
}

void fovpt_launch_focus_gather(hipStream_t st, int w, int h, int max_radius, const fovpt_float4* in, const float2* rt, fovpt_float4* out_color,
                               uint32_t* out_rgba)
{
    const dim3 grid((w + FOCUS_TW - 1) / FOCUS_TW, (h + FOCUS_TH - 1) / FOCUS_TH);
    hipLaunchKernelGGL(k_focus_gather, grid, dim3(FOCUS_TW, FOCUS_TH), 0, st, w, h, max_radius, in, rt, out_color, out_rgba);
}
