// packet.hip -- the foveated frame packet on the device (include/fovpt.h, fovpt_packet_*).
//
//   k_packet_encode    one thread per texel (launch index) of all passes in one launch: it walks the texel's clamped fill x fill
//                      block, asks find_last_writer for each pixel's last writer and averages the 8-bit codes of the pixels it
//                      owns; a plain 4-byte store per texel, and thread 0 stores the header from the argument struct.  Integer
//                      sums, no atomics, no LDS.  A fill-4 texel whose block lies inside the frame on 16-byte boundaries reads
//                      it as four 16-byte row segments: neighbouring lanes read neighbouring segments
//   k_packet_decode    one thread per pixel: the last texel with alpha != 0 whose block reaches the pixel -- find_last_writer's
//                      search (writer_range's candidates per axis, descending) with the texel's alpha where that tests the ring
//                      --, NEAREST its value, SMOOTH up to three more texels of the same pass around it
//
// The definition in integers is tests/packet_ref.py.
#include "fovpt_packet.h"
#include "fovpt_pixel.h"

namespace {

// pixel (i + k) mod 2^32 of a block along an axis of `dim` pixels, clamped onto the last one (deviceProgram.cu:554)
__device__ inline uint32_t block_pixel(uint32_t i, uint32_t k, uint32_t dim) { return min(i + k, dim - 1u); }
// an earlier pixel of the block is the same one (the clamp folds them; a wrapped block on a tiny frame can come back to it)
__device__ inline bool seen_before(uint32_t i, uint32_t k, uint32_t dim)
{
    const uint32_t px = block_pixel(i, k, dim);
    bool dup = false;
    for (uint32_t j = 0; j < k; j++) dup |= block_pixel(i, j, dim) == px;
    return dup;
}

__device__ inline uint32_t pick(const uint4& q, uint32_t u) { return u == 0u ? q.x : u == 1u ? q.y : u == 2u ? q.z : q.w; }

// vec: `in` is 16-byte aligned and the frame's width a multiple of 4
__global__ __launch_bounds__(FOVPT_BLOCK) void k_packet_encode(const FrameDev fd, const PacketArgs a, const uint32_t* __restrict__ in,
                                                               uint32_t* __restrict__ out, uint32_t vec)
{
    const uint32_t t = blockIdx.x * FOVPT_BLOCK + threadIdx.x;
    if (t == 0u) {                                                    // the header, word by word
        out[0] = a.h.magic; out[1] = a.h.version; out[2] = a.h.bytes; out[3] = a.h.sequence;
        out[4] = (uint32_t)a.h.width; out[5] = (uint32_t)a.h.height; out[6] = a.h.npass; out[7] = a.h._reserved;
#pragma unroll
        for (int p = 0; p < FOVPT_MAX_PASSES; p++) {
            const fovpt_packet_pass& P = a.h.pass[p];
            uint32_t* o = out + 8 + 8 * p;
            o[0] = P.gw; o[1] = P.gh; o[2] = P.factor; o[3] = P.fill; o[4] = P.offx; o[5] = P.offy; o[6] = P.texels; o[7] = P._reserved;
        }
    }
    if (t >= a.first[FOVPT_MAX_PASSES]) return;
    // static indices: the pass records stay in SGPRs
    const int p = t < a.first[1] ? 0 : t < a.first[2] ? 1 : 2;
    const fovpt_packet_pass& P0 = a.h.pass[0];
    const fovpt_packet_pass& P1 = a.h.pass[1];
    const fovpt_packet_pass& P2 = a.h.pass[2];
    const uint32_t gw = p == 0 ? P0.gw : p == 1 ? P1.gw : P2.gw, f = p == 0 ? P0.factor : p == 1 ? P1.factor : P2.factor;
    const uint32_t fill = p == 0 ? P0.fill : p == 1 ? P1.fill : P2.fill;
    const uint32_t offx = p == 0 ? P0.offx : p == 1 ? P1.offx : P2.offx, offy = p == 0 ? P0.offy : p == 1 ? P1.offy : P2.offy;
    const uint32_t li = t - (p == 0 ? a.first[0] : p == 1 ? a.first[1] : a.first[2]);
    const uint32_t ly = li / gw, lx = li - ly * gw;
    const uint32_t ix = lx * f + offx, iy = ly * f + offy;            // (uint32: wraps)
    const uint32_t W = (uint32_t)fd.w, H = (uint32_t)fd.h;
    // four 16-byte row segments where the block is 4 x 4, inside the frame and on 16-byte boundaries (every periphery texel
    // of a frame whose width is a multiple of 4, away from the clamped last row)
    const bool rows4 = vec && fill == 4u && !(ix & 3u) && ix < W && W - ix >= 4u && iy < H && H - iy >= 4u;
    uint4 q0 = make_uint4(0u, 0u, 0u, 0u), q1 = q0, q2 = q0, q3 = q0;
    if (rows4) {
        const uint4* r = (const uint4*)(in + (size_t)iy * W + ix);
        const size_t pitch = W >> 2;
        q0 = r[0]; q1 = r[pitch]; q2 = r[2 * pitch]; q3 = r[3 * pitch];
    }
    uint32_t n = 0u, sr = 0u, sg = 0u, sb = 0u;
#pragma unroll 1
    for (uint32_t v = 0; v < fill; v++) {
        if (seen_before(iy, v, H)) continue;
        const uint32_t py = block_pixel(iy, v, H);
        const uint4 q = v == 0u ? q0 : v == 1u ? q1 : v == 2u ? q2 : q3;
#pragma unroll 1
        for (uint32_t u = 0; u < fill; u++) {
            if (seen_before(ix, u, W)) continue;
            const uint32_t px = block_pixel(ix, u, W);
            int wp = 0;
            uint32_t wlx, wly;
            if (!find_last_writer(fd, px, py, wp, wlx, wly) || wp != p || wlx != lx || wly != ly) continue;
            const uint32_t c = rows4 ? pick(q, u) : in[(size_t)py * W + px];
            n++;
            sr += c & 0xffu; sg += (c >> 8) & 0xffu; sb += (c >> 16) & 0xffu;
        }
    }
    uint32_t texel = 0u;
    if (n) {
        const uint32_t h = n >> 1;
        texel = ((sr + h) / n) | (((sg + h) / n) << 8) | (((sb + h) / n) << 16) | 0xff000000u;
    }
    out[FOVPT_PACKET_HEADER_BYTES / 4u + t] = texel;
}

// The last texel whose block reaches pixel (x, y) and whose alpha is not 0, in the definition's write order: the highest pass,
// within it the launch index that comes last.  find_last_writer's search (fovpt_pixel.h) over the header's pass records.
__device__ inline bool find_last_texel(const PacketArgs& a, const uint32_t* __restrict__ pk, uint32_t x, uint32_t y, int& wp, uint32_t& wlx,
                                       uint32_t& wly, uint32_t& val)
{
    const uint32_t W = (uint32_t)a.h.width, H = (uint32_t)a.h.height;
#pragma unroll
    for (int p = FOVPT_MAX_PASSES - 1; p >= 0; p--) {
        if ((uint32_t)p >= a.h.npass) continue;
        const fovpt_packet_pass& P = a.h.pass[p];
        const uint32_t* tex = pk + (P.texels >> 2);
        const uint32_t f = P.factor;
        // blocks that tile the plane, away from the last column and row: one candidate per axis
        if (P.fill == f && (f & (f - 1u)) == 0u && x + 1u != W && y + 1u != H) {
            const int sh = 31 - __clz((int)f);
            const long long rx = (long long)x - (long long)(int32_t)P.offx, ry = (long long)y - (long long)(int32_t)P.offy;
            if (rx < 0 || ry < 0 || rx >= ((long long)P.gw << sh) || ry >= ((long long)P.gh << sh)) continue;
            const uint32_t lx = (uint32_t)rx >> sh, ly = (uint32_t)ry >> sh;
            const uint32_t c = tex[(size_t)ly * P.gw + lx];
            if (!(c >> 24)) continue;
            wp = p; wlx = lx; wly = ly; val = c;
            return true;
        }
        long long xa, xb, ya, yb, xw, yw;
        writer_range(x, W, f, (int)P.fill, P.offx, P.gw, xa, xb, xw);
        writer_range(y, H, f, (int)P.fill, P.offy, P.gh, ya, yb, yw);
        const long long y_end = yw >= 0 ? 0 : ya, x_end = xw >= 0 ? 0 : xa;
        // candidates in descending launch order: [ya, yb] then the wrapped rows [0, yw]; same along x
        for (long long ly = yb; ly >= y_end; ly--) {
            if (ly < ya && ly > yw) { ly = yw + 1; continue; }
            for (long long lx = xb; lx >= x_end; lx--) {
                if (lx < xa && lx > xw) { lx = xw + 1; continue; }
                const uint32_t c = tex[(size_t)ly * P.gw + (size_t)lx];
                if (!(c >> 24)) continue;
                wp = p; wlx = (uint32_t)lx; wly = (uint32_t)ly; val = c;
                return true;
            }
        }
    }
    return false;
}

template <int MODE>
__global__ __launch_bounds__(FOVPT_BLOCK) void k_packet_decode(const PacketArgs a, const uint32_t* __restrict__ pk, uint32_t* __restrict__ out)
{
    const uint32_t W = (uint32_t)a.h.width, H = (uint32_t)a.h.height;
    const uint32_t idx = blockIdx.x * FOVPT_BLOCK + threadIdx.x;      // (W * H <= 2^28)
    if (idx >= W * H) return;
    const uint32_t y = idx / W, x = idx - y * W;
    int p = 0;
    uint32_t lx, ly, val;
    if (!find_last_texel(a, pk, x, y, p, lx, ly, val)) return;        // (no texel reaches the pixel: it keeps what it held)
    if (MODE == FOVPT_PACKET_SMOOTH) {
        const fovpt_packet_pass& P0 = a.h.pass[0];
        const fovpt_packet_pass& P1 = a.h.pass[1];
        const fovpt_packet_pass& P2 = a.h.pass[2];
        const uint32_t gw = p == 0 ? P0.gw : p == 1 ? P1.gw : P2.gw, gh = p == 0 ? P0.gh : p == 1 ? P1.gh : P2.gh;
        const uint32_t f = p == 0 ? P0.factor : p == 1 ? P1.factor : P2.factor, fill = p == 0 ? P0.fill : p == 1 ? P1.fill : P2.fill;
        const uint32_t offx = p == 0 ? P0.offx : p == 1 ? P1.offx : P2.offx, offy = p == 0 ? P0.offy : p == 1 ? P1.offy : P2.offy;
        const uint32_t* tex = pk + ((p == 0 ? P0.texels : p == 1 ? P1.texels : P2.texels) >> 2);
        const uint32_t ix = lx * f + offx, iy = ly * f + offy;        // the block's anchor (uint32: wraps)
        const uint32_t rx = x - ix, ry = y - iy;
        if (fill == f && fill > 1u && x >= ix && rx < fill && y >= iy && ry < fill) {      // a regular pixel
            const int dx = 2 * (int)rx + 1 - (int)fill, dy = 2 * (int)ry + 1 - (int)fill;
            const int sx = dx > 0 ? 1 : -1, sy = dy > 0 ? 1 : -1;
            const uint32_t nx = (uint32_t)abs(dx), ny = (uint32_t)abs(dy), ox = 2u * fill - nx, oy = 2u * fill - ny;
            const long long tx = (long long)lx + sx, ty = (long long)ly + sy;
            const bool inx = tx >= 0 && tx < (long long)gw, iny = ty >= 0 && ty < (long long)gh;
            // the loads first: up to three of them in flight
            const uint32_t cx = inx ? tex[(size_t)ly * gw + (size_t)tx] : 0u;
            const uint32_t cy = iny ? tex[(size_t)ty * gw + lx] : 0u;
            const uint32_t cd = inx && iny ? tex[(size_t)ty * gw + (size_t)tx] : 0u;
            const uint32_t w0 = ox * oy, w1 = (cx >> 24) ? nx * oy : 0u, w2 = (cy >> 24) ? ox * ny : 0u, w3 = (cd >> 24) ? nx * ny : 0u;
            const uint32_t Wt = w0 + w1 + w2 + w3, half = Wt >> 1;   // (Wt >= (fill + 1)^2 > 0; at most 256)
            uint32_t o = 0xff000000u;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const uint32_t s = w0 * ((val >> (8 * k)) & 0xffu) + w1 * ((cx >> (8 * k)) & 0xffu) + w2 * ((cy >> (8 * k)) & 0xffu)
                                   + w3 * ((cd >> (8 * k)) & 0xffu);
                o |= ((s + half) / Wt) << (8 * k);
            }
            val = o;
        }
    }
    out[idx] = val;
}

}  // namespace

void fovpt_launch_packet_encode(hipStream_t st, const FrameDev& fd, const PacketArgs& a, const uint32_t* in, uint32_t* out)
{
    const uint32_t total = a.first[FOVPT_MAX_PASSES];                 // (>= 1: every pass has a launch index)
    const uint32_t vec = ((uintptr_t)in & 15u) == 0u && (fd.w & 3) == 0 ? 1u : 0u;
    hipLaunchKernelGGL(k_packet_encode, dim3((total + FOVPT_BLOCK - 1) / FOVPT_BLOCK), dim3(FOVPT_BLOCK), 0, st, fd, a, in, out, vec);
}

void fovpt_launch_packet_decode(hipStream_t st, const PacketArgs& a, int mode, const uint32_t* packet, uint32_t* out)
{
    const uint32_t npix = (uint32_t)a.h.width * (uint32_t)a.h.height;
    const dim3 grid((npix + FOVPT_BLOCK - 1) / FOVPT_BLOCK);
    if (mode == FOVPT_PACKET_SMOOTH) hipLaunchKernelGGL(k_packet_decode<FOVPT_PACKET_SMOOTH>, grid, dim3(FOVPT_BLOCK), 0, st, a, packet, out);
    else hipLaunchKernelGGL(k_packet_decode<FOVPT_PACKET_NEAREST>, grid, dim3(FOVPT_BLOCK), 0, st, a, packet, out);
}
