// expose.hip -- fovpt_expose: gaze-metered auto-exposure and tone map of a frame.
//
//   k_expose_meter   the weighted log-luminance histogram of the input: 8 bins per octave over 2^-16 .. 2^16 from the bits of the
//                    luminance (integer operations only), the weight of a pixel by the fill of its last writer (METER_GAZE) or 1
//                    (METER_FRAME).  Grid-stride; one LDS copy of the histogram per wave, summed at the end; a block stores its
//                    256 counts as one row of a [blocks][256] buffer.  No global atomics: integer sums, any order, same result
//   k_expose_adapt   one block: the column sums of those rows in 64 bits (the histogram), a scan in LDS, the trimmed mean of the bin
//                    centres between two ranks, the adaptation step and the exposure, into the device state record
//   k_expose_apply   per pixel: the tone map at that exposure (read from the state record, or an argument: EXPOSE_FIXED)
//
// The definition, operation by operation, is tests/expose_ref.py; -ffp-contract=off keeps every product and sum of it a
// separate binary32 (binary64 in the trimmed mean) op.
#include "fovpt_device.h"
#include "fovpt_pixel.h"

namespace {

#define EXPOSE_BINS FOVPT_EXPOSE_BINS
#define EXPOSE_WAVES (FOVPT_EXPOSE_BLOCK / FOVPT_WAVE)
#define EXPOSE_UNROLL 4                 // pixels a thread of the meter has in flight
static_assert(EXPOSE_BINS <= FOVPT_EXPOSE_BLOCK && FOVPT_EXPOSE_BLOCK % EXPOSE_BINS == 0 && EXPOSE_BINS == 4 * FOVPT_WAVE, "a thread per bin, a wave per row");

// GAZE: a pixel's weight by the foveation level of its last writer (by_level, fovpt_pixel.h)
template <bool GAZE>
__global__ __launch_bounds__(FOVPT_EXPOSE_BLOCK) void k_expose_meter(const FrameDev fd, const ExposeArgs a, uint32_t npix,
                                                                     const fovpt_float4* __restrict__ in, uint32_t* __restrict__ rows)
{
    __shared__ uint32_t h[EXPOSE_WAVES][EXPOSE_BINS];                // a rendered frame puts most pixels in a few bins: a copy per wave
    const uint32_t t = threadIdx.x, wave = t / FOVPT_WAVE;
    for (uint32_t k = t; k < EXPOSE_WAVES * EXPOSE_BINS; k += FOVPT_EXPOSE_BLOCK) (&h[0][0])[k] = 0u;
    __syncthreads();
    const uint32_t stride = gridDim.x * FOVPT_EXPOSE_BLOCK, w = (uint32_t)fd.w;
    // (npix < 2^31 and stride <= 2^19: no index below wraps)
    for (uint32_t i0 = blockIdx.x * FOVPT_EXPOSE_BLOCK + t; i0 < npix; i0 += EXPOSE_UNROLL * stride) {
        float L[EXPOSE_UNROLL];
#pragma unroll
        for (int j = 0; j < EXPOSE_UNROLL; j++) {                     // the loads first: EXPOSE_UNROLL of them in flight
            const uint32_t idx = i0 + (uint32_t)j * stride;
            L[j] = idx < npix ? luma(v3(in[idx])) : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < EXPOSE_UNROLL; j++) {
            const uint32_t idx = i0 + (uint32_t)j * stride;
            if (!(L[j] > 0.0f)) continue;                             // (+inf counts; NaN, 0 and negatives do not; nor does idx >= npix)
            uint32_t wgt = 1u;
            if (GAZE) {
                const uint32_t y = idx / w, x = idx - y * w;
                int wp = 0;
                uint32_t wlx, wly;
                if (!find_last_writer(fd, x, y, wp, wlx, wly)) continue;
                wgt = (uint32_t)by_level(a.weight, a.uniform, fd.pass[wp].fill);
                if (!wgt) continue;
            }
            const int bin = min(max((int)(__float_as_uint(L[j]) >> 20) - 888, 0), EXPOSE_BINS - 1);
            atomicAdd(&h[wave][bin], wgt);                            // (a block's pixels * 255 < 2^32: fovpt_expose_rows)
        }
    }
    __syncthreads();
    if (t >= EXPOSE_BINS) return;
    uint32_t s = 0u;
    for (uint32_t k = 0; k < EXPOSE_WAVES; k++) s += h[k][t];
    rows[(size_t)blockIdx.x * EXPOSE_BINS + t] = s;
}

__global__ __launch_bounds__(FOVPT_EXPOSE_BLOCK) void k_expose_adapt(const ExposeArgs a, const uint32_t* __restrict__ rows, uint32_t nrows,
                                                                     uint64_t* __restrict__ hist, ExposeState* __restrict__ state)
{
    __shared__ uint64_t part[EXPOSE_WAVES][EXPOSE_BINS];
    __shared__ uint64_t cum[2][EXPOSE_BINS];
    __shared__ uint64_t cut[2];
    const uint32_t k = threadIdx.x, lane = k % FOVPT_WAVE, wave = k / FOVPT_WAVE;
    const bool own = k < EXPOSE_BINS;                                 // thread k < 256 owns bin k; the others only help with the rows
    // the column sums: a wave reads a whole row with one 16-byte load per lane (bins 4 lane .. 4 lane + 3), the waves take the
    // rows in turn (one block has to pull every row through one CU: few, wide loads, all of a wave's in flight together)
    uint64_t acc[4] = {0ull, 0ull, 0ull, 0ull};
    const uint4* rows4 = (const uint4*)rows;
#pragma unroll 8
    for (uint32_t r = wave; r < nrows; r += EXPOSE_WAVES) {
        const uint4 q = rows4[(size_t)r * (EXPOSE_BINS / 4) + lane];
        acc[0] += q.x; acc[1] += q.y; acc[2] += q.z; acc[3] += q.w;
    }
    for (int j = 0; j < 4; j++) part[wave][4 * lane + j] = acc[j];
    __syncthreads();
    uint64_t hk = 0ull;
    if (own) {
        for (uint32_t v = 0; v < EXPOSE_WAVES; v++) hk += part[v][k];
        hist[k] = hk;
        cum[0][k] = hk;
    }
    // inclusive scan (Hillis-Steele, two buffers)
    int cur = 0;
    __syncthreads();
    for (uint32_t d = 1; d < EXPOSE_BINS; d <<= 1) {
        if (own) cum[cur ^ 1][k] = cum[cur][k] + (k >= d ? cum[cur][k - d] : 0ull);
        cur ^= 1;
        __syncthreads();
    }
    const uint64_t hi = own ? cum[cur][k] : 0ull, lo = hi - hk, T = cum[cur][EXPOSE_BINS - 1];
    if (k == 0) {
        cut[0] = T * (uint64_t)a.low / 1000ull;                       // (T < 2^39: the products fit)
        cut[1] = (T * (uint64_t)a.high + 999ull) / 1000ull;
    }
    __syncthreads();
    const uint64_t ca = cut[0], cb = cut[1];
    const uint64_t top = hi < cb ? hi : cb, bot = lo > ca ? lo : ca;
    const uint64_t ck = top > bot ? top - bot : 0ull;
    __syncthreads();                                                  // (every thread has read its cum entries)
    if (own) cum[0][k] = ck * (uint64_t)(2u * k + 1u);
    __syncthreads();
    for (uint32_t d = EXPOSE_BINS / 2; d >= 1; d >>= 1) {             // fixed-order tree
        if (k < d) cum[0][k] += cum[0][k + d];
        __syncthreads();
    }
    if (k != 0) return;
    const uint64_t S = cum[0][0], N = cb - ca;
    const bool first = state->steps == 0ull;
    float ev = state->ev, target;
    if (N != 0ull) {
        const double m = -16.0 + ((double)S / (2.0 * (double)N)) / 8.0;
        target = (float)fmax((double)a.ev_min, fmin(m, (double)a.ev_max));
    } else target = first ? fmaxf(a.ev_min, fminf(0.0f, a.ev_max)) : ev;
    if (first) ev = target;
    else {
        const float rate = target > ev ? a.adapt_brighter : a.adapt_darker;
        ev = ev + rate * (target - ev);
    }
    state->ev_metered = target;
    state->ev = ev;
    state->exposure = a.key / fovpt_dm_powf(2.0f, ev);
    state->_pad = 0.0f;
    state->weight_total = T;
    state->steps = state->steps + 1ull;
}

__device__ inline float aces1(float x) { return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f); }

// `in` and `out_color` may be the same buffer: a thread reads only its own pixel of `in`, before it writes out_color
__global__ __launch_bounds__(FOVPT_BLOCK) void k_expose_apply(const ExposeArgs a, uint32_t npix, const ExposeState* __restrict__ state,
                                                              const fovpt_float4* in, fovpt_float4* out_color, uint32_t* __restrict__ out_rgba)
{
    const uint32_t idx = blockIdx.x * FOVPT_BLOCK + threadIdx.x;
    if (idx >= npix) return;
    const float E = state ? state->exposure : a.exposure;
    const fovpt_float4 c = in[idx];
    const V3 x = v3(c.x, c.y, c.z) * E;
    const V3 o = a.tone == FOVPT_TONE_ACES ? v3(aces1(x.x), aces1(x.y), aces1(x.z)) : reinhard(x, a.white);
    out_color[idx] = fovpt_float4{o.x, o.y, o.z, 1.0f};
    out_rgba[idx] = make_color(o);
}

}  // namespace

uint32_t fovpt_expose_rows(size_t npix)
{
    const size_t blocks = (npix + FOVPT_EXPOSE_BLOCK - 1) / FOVPT_EXPOSE_BLOCK;
    return (uint32_t)(blocks < FOVPT_EXPOSE_MAX_ROWS ? blocks : FOVPT_EXPOSE_MAX_ROWS);
}

void fovpt_launch_expose_meter(hipStream_t st, const FrameDev& fd, const ExposeArgs& a, bool gaze, const fovpt_float4* in, uint32_t* rows)
{
    const size_t npix = (size_t)fd.w * (size_t)fd.h;
    const dim3 grid(fovpt_expose_rows(npix));
    if (gaze) hipLaunchKernelGGL(k_expose_meter<true>, grid, dim3(FOVPT_EXPOSE_BLOCK), 0, st, fd, a, (uint32_t)npix, in, rows);
    else hipLaunchKernelGGL(k_expose_meter<false>, grid, dim3(FOVPT_EXPOSE_BLOCK), 0, st, fd, a, (uint32_t)npix, in, rows);
}

void fovpt_launch_expose_adapt(hipStream_t st, const ExposeArgs& a, const uint32_t* rows, uint32_t nrows, uint64_t* hist, ExposeState* state)
{
    hipLaunchKernelGGL(k_expose_adapt, dim3(1), dim3(FOVPT_EXPOSE_BLOCK), 0, st, a, rows, nrows, hist, state);
}

void fovpt_launch_expose_apply(hipStream_t st, size_t npix, const ExposeArgs& a, const ExposeState* state, const fovpt_float4* in,
                               fovpt_float4* out_color, uint32_t* out_rgba)
{
    const dim3 grid((uint32_t)((npix + FOVPT_BLOCK - 1) / FOVPT_BLOCK));
    hipLaunchKernelGGL(k_expose_apply, grid, dim3(FOVPT_BLOCK), 0, st, a, (uint32_t)npix, state, in, out_color, out_rgba);
}
