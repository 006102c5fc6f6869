// quality.hip -- fovpt_quality: per-level error sums, SSIM and eccentricity profile of two rgba8 images of the rendered frame
// (DESIGN.md, section 31).
//
//   k_quality_tile   a block of 256 threads owns a 32 x 32 pixel tile, and strides over the tiles.  A thread takes four pixels
//                    of a row (one 16-byte load per image where the frame allows it): the class of each by find_last_writer, the
//                    error sums, the ring, and the two lumas into LDS; 68 threads add the lumas of the 4-pixel apron right of and
//                    below the tile.  81 threads form the sums sx, sy, sxx, syy, sxy of the 4 x 4 pixel cells of that 36 x 36
//                    region once, 64 threads each put a window together from 2 x 2 cells (the tile owns the windows whose origin
//                    lies in it: origins are multiples of 4, so a window reaches 4 pixels past the tile, not 7) and take the
//                    class of its centre pixel from LDS (from a search of its own where the centre lies in the next tile).
//                    Sums of a tile live in LDS as 32-bit integers (LDS atomics; a thread first adds up its run of equal classes
//                    and rings in registers); after each tile thread k adds column k to a 64-bit register and clears it; a block
//                    stores its FOVPT_QUALITY_COLUMNS registers as one row of a [blocks][columns] buffer.
//   k_quality_sum    one block: the column sums of those rows in 64 bits (the maximum for max_err), every byte of the record.
//
// No global atomics and no floating-point accumulation: integer sums in any order give the same result.  The one floating-point
// value, a window's q, is a binary64 quotient of two exact integers, rounded to an integer before it is added.  The definition,
// operation by operation, is tests/quality_ref.py.
#include "fovpt_device.h"
#include "fovpt_pixel.h"

namespace {

#define Q_TILE FOVPT_QUALITY_TILE
#define Q_BLOCK FOVPT_QUALITY_BLOCK
#define Q_WAVES (Q_BLOCK / FOVPT_WAVE)
#define Q_COLS FOVPT_QUALITY_COLUMNS
#define Q_CLASSES FOVPT_QUALITY_CLASSES
#define Q_RINGS FOVPT_QUALITY_RINGS
#define Q_REGION_WORDS ((Q_TILE + 4) / 4)                  // a row of the 36 x 36 luma region: 9 words of 4 lumas
#define Q_CELLS (Q_TILE / 4 + 1)                           // 4 x 4 pixel cells along a side of the region: 9
#define Q_SUM_WAVES (FOVPT_QUALITY_SUM_BLOCK / FOVPT_WAVE)
// the columns of a row: per class pixels, differing, sq_err r g b, max_err, windows, ssim_q20; then the rings' pixels and sq_err
enum { COL_PIXELS = 0, COL_DIFFERING = Q_CLASSES, COL_SQ_ERR = 2 * Q_CLASSES, COL_MAX_ERR = 5 * Q_CLASSES, COL_WINDOWS = 6 * Q_CLASSES,
       COL_SSIM = 7 * Q_CLASSES, COL_RING_PIXELS = 8 * Q_CLASSES, COL_RING_SQ_ERR = 8 * Q_CLASSES + Q_RINGS };
static_assert(Q_TILE == 32 && Q_BLOCK == 256 && Q_BLOCK * 4 == Q_TILE * Q_TILE, "a thread per four pixels of a tile row");
static_assert(Q_COLS <= Q_BLOCK && Q_COLS <= 3 * FOVPT_WAVE && Q_COLS + 1 <= FOVPT_QUALITY_SUM_BLOCK, "a thread per column");
static_assert(COL_RING_SQ_ERR + Q_RINGS == Q_COLS && COL_MAX_ERR + Q_CLASSES <= FOVPT_WAVE, "the columns");

// (not by_level, fovpt_pixel.h: a class table picked with it changes the machine code of every k_quality_tile)
__device__ inline uint32_t quality_class(const FrameDev& fd, bool uniform, uint32_t x, uint32_t y)
{
    int wp = 0;
    uint32_t wlx, wly;
    if (!find_last_writer(fd, x, y, wp, wlx, wly)) return FOVPT_QUALITY_UNWRITTEN;
    if (uniform) return FOVPT_QUALITY_UNIFORM;
    int f = 0;
#pragma unroll
    for (int p = 0; p < FOVPT_MAX_PASSES; p++) f = wp == p ? fd.pass[p].fill : f;   // static indices: the pass records stay in SGPRs
    return f == 4 ? FOVPT_QUALITY_PERIPHERY : f == 2 ? FOVPT_QUALITY_MIDDLE : FOVPT_QUALITY_FOVEA;
}

// min(63, isqrt(dx^2 + dy^2) / ring_width).  |dx| or |dy| >= 2^22 is ring 63 without the square (isqrt >= 2^22 > 63 *
// FOVPT_QUALITY_MAX_RING_WIDTH); below that d2 < 2^45 is exact as a binary64, and its square root, whatever its last bit, is
// corrected to the exact floor in integers
__device__ inline uint32_t quality_ring(int64_t dx, int64_t dy, uint32_t ring_width)
{
    const uint64_t ax = (uint64_t)(dx < 0 ? -dx : dx), ay = (uint64_t)(dy < 0 ? -dy : dy);
    if (ax >= (1ull << 22) || ay >= (1ull << 22)) return Q_RINGS - 1;
    const uint64_t d2 = ax * ax + ay * ay;
    uint64_t r = (uint64_t)sqrt((double)d2);
    while (r * r > d2) r--;
    while ((r + 1ull) * (r + 1ull) <= d2) r++;
    return min((uint32_t)r / ring_width, (uint32_t)(Q_RINGS - 1));       // (r < 2^23: a 32-bit division)
}

__device__ inline uint32_t luma8(uint32_t p) { return (54u * (p & 255u) + 183u * ((p >> 8) & 255u) + 19u * ((p >> 16) & 255u) + 128u) >> 8; }

// four pixels of a row from x on, 0 beyond the frame.  vec: the images are 16-byte aligned and w is a multiple of 4, so the four
// (x is one too) are one aligned 16-byte word and lie in the frame together
__device__ inline void load4(const uint32_t* img, bool vec, uint32_t w, uint32_t h, uint32_t x, uint32_t y, uint32_t p[4])
{
    p[0] = p[1] = p[2] = p[3] = 0u;
    if (y >= h || x >= w) return;
    const size_t i = (size_t)y * w + x;
    if (vec) {
        const uint4 q = *(const uint4*)(img + i);
        p[0] = q.x; p[1] = q.y; p[2] = q.z; p[3] = q.w;
        return;
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; j++)
        if (x + j < w) p[j] = img[i + j];
}

// vec bit 0: load4's; bit 1: out_class is 4-byte aligned and w a multiple of 4 (a thread's four classes are one store)
template <bool SSIM, bool PROFILE>
__global__ __launch_bounds__(Q_BLOCK) void k_quality_tile(const FrameDev fd, const QualityArgs a, uint32_t tiles_x, uint32_t ntiles, int vec,
                                                          const uint32_t* test, const uint32_t* ref, uint64_t* __restrict__ rows,
                                                          uint8_t* __restrict__ out_class)
{
    // a 1024-pixel tile keeps every 32-bit partial below 2^32: sq_err of a channel <= 1024 * 255^2 < 2^26, of a ring (three
    // channels) < 2^28, |ssim_q20| <= 64 windows * 2^20 = 2^26
    __shared__ uint32_t csum[8 * Q_CLASSES];
    __shared__ uint32_t ring[Q_WAVES][2 * Q_RINGS];                  // a copy per wave: near the gaze a tile is one ring
    __shared__ uint32_t luma_t[(Q_TILE + 4) * Q_REGION_WORDS], luma_f[(Q_TILE + 4) * Q_REGION_WORDS];   // four lumas a word
    __shared__ uint32_t cls4[Q_TILE * Q_TILE / 4];                   // the tile's classes, four a word
    __shared__ uint32_t cell[5][Q_CELLS * Q_CELLS];
    const uint32_t t = threadIdx.x, wave = t / FOVPT_WAVE;
    const uint32_t w = (uint32_t)fd.w, h = (uint32_t)fd.h;
    const bool uniform = a.uniform != 0, vec_in = (vec & 1) != 0, vec_cls = (vec & 2) != 0;
    if (t < 8 * Q_CLASSES) csum[t] = 0u;
    for (uint32_t k = t; k < Q_WAVES * 2 * Q_RINGS; k += Q_BLOCK) (&ring[0][0])[k] = 0u;
    uint64_t acc = 0ull;                                             // column t of this block's row
    __syncthreads();
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t tyi = tile / tiles_x, X0 = (tile - tyi * tiles_x) * Q_TILE, Y0 = tyi * Q_TILE;
        // ---- the thread's four pixels: row t / 8 of the tile, columns 4 (t % 8) .. + 3
        const uint32_t ly = t >> 3, y = Y0 + ly, x0 = X0 + ((t & 7u) << 2);
        uint32_t T[4], F[4];
        load4(test, vec_in, w, h, x0, y, T);
        load4(ref, vec_in, w, h, x0, y, F);
        uint32_t cur = 0xffffffffu, n = 0u, nd = 0u, s0 = 0u, s1 = 0u, s2 = 0u, mx = 0u;   // the run of one class
        uint32_t cur_ring = 0xffffffffu, rn = 0u, rs = 0u;                                   // the run of one ring
        uint32_t lt = 0u, lf = 0u, kw = 0u;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            if (y >= h || x0 + j >= w) continue;
            const uint32_t k = quality_class(fd, uniform, x0 + j, y);
            const int32_t d0 = (int32_t)(T[j] & 255u) - (int32_t)(F[j] & 255u), d1 = (int32_t)((T[j] >> 8) & 255u) - (int32_t)((F[j] >> 8) & 255u),
                          d2 = (int32_t)((T[j] >> 16) & 255u) - (int32_t)((F[j] >> 16) & 255u);
            const uint32_t a0 = (uint32_t)abs(d0), a1 = (uint32_t)abs(d1), a2 = (uint32_t)abs(d2), m = max(a0, max(a1, a2));
            if (k != cur) {
                if (n) {
                    atomicAdd(&csum[COL_PIXELS + cur], n); atomicAdd(&csum[COL_DIFFERING + cur], nd);
                    atomicAdd(&csum[COL_SQ_ERR + 3u * cur], s0); atomicAdd(&csum[COL_SQ_ERR + 3u * cur + 1u], s1); atomicAdd(&csum[COL_SQ_ERR + 3u * cur + 2u], s2);
                    atomicMax(&csum[COL_MAX_ERR + cur], mx);
                }
                cur = k; n = nd = s0 = s1 = s2 = mx = 0u;
            }
            n++; nd += m != 0u; s0 += a0 * a0; s1 += a1 * a1; s2 += a2 * a2; mx = max(mx, m);
            if (PROFILE) {
                const uint32_t r = quality_ring((int64_t)(x0 + j) - a.cx, (int64_t)y - a.cy, (uint32_t)a.ring_width);
                if (r != cur_ring) {
                    if (rn) { atomicAdd(&ring[wave][cur_ring], rn); atomicAdd(&ring[wave][Q_RINGS + cur_ring], rs); }
                    cur_ring = r; rn = rs = 0u;
                }
                rn++; rs += (a0 * a0 + a1 * a1) + a2 * a2;
            }
            if (SSIM) { lt |= luma8(T[j]) << (8u * j); lf |= luma8(F[j]) << (8u * j); }
            kw |= k << (8u * j);
        }
        if (n) {
            atomicAdd(&csum[COL_PIXELS + cur], n); atomicAdd(&csum[COL_DIFFERING + cur], nd);
            atomicAdd(&csum[COL_SQ_ERR + 3u * cur], s0); atomicAdd(&csum[COL_SQ_ERR + 3u * cur + 1u], s1); atomicAdd(&csum[COL_SQ_ERR + 3u * cur + 2u], s2);
            atomicMax(&csum[COL_MAX_ERR + cur], mx);
        }
        if (PROFILE && rn) { atomicAdd(&ring[wave][cur_ring], rn); atomicAdd(&ring[wave][Q_RINGS + cur_ring], rs); }
        if (out_class && y < h && x0 < w) {
            const size_t i = (size_t)y * w + x0;
            if (vec_cls) *(uint32_t*)(out_class + i) = kw;
            else {
#pragma unroll
                for (uint32_t j = 0; j < 4; j++)
                    if (x0 + j < w) out_class[i + j] = (uint8_t)(kw >> (8u * j));
            }
        }
        if (SSIM) {
            luma_t[ly * Q_REGION_WORDS + (t & 7u)] = lt; luma_f[ly * Q_REGION_WORDS + (t & 7u)] = lf;
            cls4[t] = kw;
            // the apron: word 8 of rows 0 .. 35, then words 0 .. 7 of rows 32 .. 35 (pixels beyond the frame: 0, and in no window)
            if (t < (Q_TILE + 4) + 4 * (Q_TILE / 4)) {
                const uint32_t ry = t < Q_TILE + 4 ? t : Q_TILE + ((t - (Q_TILE + 4)) >> 3), rw = t < Q_TILE + 4 ? Q_TILE / 4 : (t - (Q_TILE + 4)) & 7u;
                uint32_t P[4], Q[4];
                load4(test, vec_in, w, h, X0 + 4u * rw, Y0 + ry, P);
                load4(ref, vec_in, w, h, X0 + 4u * rw, Y0 + ry, Q);
                uint32_t pt = 0u, pf = 0u;
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) { pt |= luma8(P[j]) << (8u * j); pf |= luma8(Q[j]) << (8u * j); }
                luma_t[ry * Q_REGION_WORDS + rw] = pt; luma_f[ry * Q_REGION_WORDS + rw] = pf;
            }
            __syncthreads();
            // ---- the 4 x 4 pixel cells of the region: a thread each
            if (t < Q_CELLS * Q_CELLS) {
                const uint32_t by = t / Q_CELLS, bx = t - by * Q_CELLS;
                uint32_t sx = 0u, sy = 0u, sxx = 0u, syy = 0u, sxy = 0u;      // (16 pixels: sxx <= 16 * 255^2 < 2^21)
#pragma unroll
                for (uint32_t r = 0; r < 4; r++) {
                    const uint32_t wt = luma_t[(4u * by + r) * Q_REGION_WORDS + bx], wf = luma_f[(4u * by + r) * Q_REGION_WORDS + bx];
#pragma unroll
                    for (uint32_t j = 0; j < 4; j++) {
                        const uint32_t p = (wt >> (8u * j)) & 255u, q = (wf >> (8u * j)) & 255u;
                        sx += p; sy += q; sxx += p * p; syy += q * q; sxy += p * q;
                    }
                }
                cell[0][t] = sx; cell[1][t] = sy; cell[2][t] = sxx; cell[3][t] = syy; cell[4][t] = sxy;
            }
            __syncthreads();
            // ---- the windows whose origin lies in the tile: a thread each, 2 x 2 cells
            if (t < (Q_TILE / 4) * (Q_TILE / 4)) {
                const uint32_t wj = t >> 3, wi = t & 7u, gx = X0 + 4u * wi, gy = Y0 + 4u * wj;
                if (gx + 8u <= w && gy + 8u <= h) {
                    const uint32_t b = wj * Q_CELLS + wi;
                    int64_t s[5];
#pragma unroll
                    for (int v = 0; v < 5; v++) s[v] = (int64_t)((cell[v][b] + cell[v][b + 1u]) + (cell[v][b + Q_CELLS] + cell[v][b + Q_CELLS + 1u]));
                    const int64_t sx = s[0], sy = s[1], sxx = s[2], syy = s[3], sxy = s[4], C1 = 26634, C2 = 239708;
                    const int64_t A = 2 * sx * sy + C1, B = 2 * (64 * sxy - sx * sy) + C2, C = sx * sx + sy * sy + C1,
                                  D = (64 * sxx - sx * sx) + (64 * syy - sy * sy) + C2;
                    const int64_t N = A * B, M = C * D;                      // (|N|, M < 2^57; M > 0)
                    const double quot = __ll2double_rn(N) / __ll2double_rn(M);
                    const int32_t q = (int32_t)rint(quot * 1048576.0);       // (|q| <= 2^20)
                    const uint32_t cxl = 4u * wi + 4u, cyl = 4u * wj + 4u;   // the centre pixel: in this tile, or the first of the next
                    const uint32_t k = cxl < Q_TILE && cyl < Q_TILE ? (cls4[(cyl * Q_TILE + cxl) >> 2] >> (8u * (cxl & 3u))) & 255u
                                                                     : quality_class(fd, uniform, gx + 4u, gy + 4u);
                    atomicAdd(&csum[COL_WINDOWS + k], 1u);
                    atomicAdd((int32_t*)&csum[COL_SSIM + k], q);
                }
            }
        }
        __syncthreads();
        // ---- the tile's sums into the block's 64-bit columns
        if (t < Q_COLS) {
            uint32_t v = 0u;
            if (t < 8 * Q_CLASSES) { v = csum[t]; csum[t] = 0u; }
            else if (PROFILE) {
#pragma unroll
                for (uint32_t k = 0; k < Q_WAVES; k++) { v += ring[k][t - 8 * Q_CLASSES]; ring[k][t - 8 * Q_CLASSES] = 0u; }
            }
            if (t >= COL_MAX_ERR && t < COL_MAX_ERR + Q_CLASSES) acc = max(acc, (uint64_t)v);
            else if (t >= COL_SSIM && t < COL_SSIM + Q_CLASSES) acc += (uint64_t)(int64_t)(int32_t)v;
            else acc += (uint64_t)v;
        }
        __syncthreads();
    }
    if (t < Q_COLS) rows[(size_t)blockIdx.x * Q_COLS + t] = acc;
}

__global__ __launch_bounds__(FOVPT_QUALITY_SUM_BLOCK) void k_quality_sum(const QualityArgs a, uint32_t w, uint32_t h, const uint64_t* __restrict__ rows,
                                                                         uint32_t nrows, fovpt_quality_sums* __restrict__ out)
{
    __shared__ uint64_t part[Q_SUM_WAVES][Q_COLS];
    const uint32_t k = threadIdx.x, lane = k % FOVPT_WAVE, wave = k / FOVPT_WAVE;
    // a wave reads a whole row with three 8-byte loads per lane (columns lane, lane + 64, lane + 128), the waves take the rows in
    // turn; the max_err columns are all among the first 64
    const bool is_max = lane >= COL_MAX_ERR && lane < COL_MAX_ERR + Q_CLASSES;
    uint64_t acc[3] = {0ull, 0ull, 0ull};
#pragma unroll 4
    for (uint32_t r = wave; r < nrows; r += Q_SUM_WAVES) {
        const uint64_t* row = rows + (size_t)r * Q_COLS;
        const uint64_t v0 = row[lane], v1 = row[lane + FOVPT_WAVE], v2 = lane + 2 * FOVPT_WAVE < Q_COLS ? row[lane + 2 * FOVPT_WAVE] : 0ull;
        acc[0] = is_max ? max(acc[0], v0) : acc[0] + v0;
        acc[1] += v1; acc[2] += v2;
    }
    part[wave][lane] = acc[0]; part[wave][lane + FOVPT_WAVE] = acc[1];
    if (lane + 2 * FOVPT_WAVE < Q_COLS) part[wave][lane + 2 * FOVPT_WAVE] = acc[2];
    __syncthreads();
    if (k == Q_COLS) {                                                 // the fields that are no sums
        out->_pad = 0u;
        out->width = w; out->height = h; out->ring_width = (uint32_t)a.ring_width; out->flags = (uint32_t)a.flags;
    }
    if (k >= Q_COLS) return;
    const bool kmax = k >= COL_MAX_ERR && k < COL_MAX_ERR + Q_CLASSES;
    uint64_t v = 0ull;
    for (uint32_t i = 0; i < Q_SUM_WAVES; i++) v = kmax ? max(v, part[i][k]) : v + part[i][k];
    if (k < COL_DIFFERING) out->pixels[k] = v;
    else if (k < COL_SQ_ERR) out->differing[k - COL_DIFFERING] = v;
    else if (k < COL_MAX_ERR) out->sq_err[(k - COL_SQ_ERR) / 3u][(k - COL_SQ_ERR) % 3u] = v;
    else if (k < COL_WINDOWS) out->max_err[k - COL_MAX_ERR] = (uint32_t)v;
    else if (k < COL_SSIM) out->windows[k - COL_WINDOWS] = v;
    else if (k < COL_RING_PIXELS) out->ssim_q20[k - COL_SSIM] = (int64_t)v;
    else if (k < COL_RING_SQ_ERR) out->ring_pixels[k - COL_RING_PIXELS] = v;
    else out->ring_sq_err[k - COL_RING_SQ_ERR] = v;
}

}  // namespace

uint32_t fovpt_quality_rows(int w, int h)
{
    const size_t tiles = (((size_t)w + Q_TILE - 1) / Q_TILE) * (((size_t)h + Q_TILE - 1) / Q_TILE);
    return (uint32_t)(tiles < FOVPT_QUALITY_MAX_ROWS ? tiles : FOVPT_QUALITY_MAX_ROWS);
}

void fovpt_launch_quality(hipStream_t st, const FrameDev& fd, const QualityArgs& a, const uint32_t* test, const uint32_t* ref, uint64_t* rows,
                          fovpt_quality_sums* out_sums, uint8_t* out_class)
{
    const uint32_t tiles_x = ((uint32_t)fd.w + Q_TILE - 1) / Q_TILE, ntiles = tiles_x * (((uint32_t)fd.h + Q_TILE - 1) / Q_TILE);   // (w h < 2^31)
    const uint32_t nrows = fovpt_quality_rows(fd.w, fd.h);
    const bool w4 = (fd.w & 3) == 0;
    const int vec = (w4 && (((uintptr_t)test | (uintptr_t)ref) & 15u) == 0 ? 1 : 0) | (w4 && ((uintptr_t)out_class & 3u) == 0 ? 2 : 0);
    const dim3 grid(nrows), block(Q_BLOCK);
    const bool ssim = (a.flags & FOVPT_QUALITY_SSIM) != 0, profile = (a.flags & FOVPT_QUALITY_PROFILE) != 0;
    if (ssim && profile) hipLaunchKernelGGL((k_quality_tile<true, true>), grid, block, 0, st, fd, a, tiles_x, ntiles, vec, test, ref, rows, out_class);
    else if (ssim) hipLaunchKernelGGL((k_quality_tile<true, false>), grid, block, 0, st, fd, a, tiles_x, ntiles, vec, test, ref, rows, out_class);
    else if (profile) hipLaunchKernelGGL((k_quality_tile<false, true>), grid, block, 0, st, fd, a, tiles_x, ntiles, vec, test, ref, rows, out_class);
    else hipLaunchKernelGGL((k_quality_tile<false, false>), grid, block, 0, st, fd, a, tiles_x, ntiles, vec, test, ref, rows, out_class);
    hipLaunchKernelGGL(k_quality_sum, dim3(1), dim3(FOVPT_QUALITY_SUM_BLOCK), 0, st, a, (uint32_t)fd.w, (uint32_t)fd.h, rows, nrows, out_sums);
}
