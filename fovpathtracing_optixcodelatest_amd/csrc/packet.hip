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
//   k_packet_encode_coded  the same texels as a coded packet ("FVPC"): per pass raw, or BC1 blocks of 4 x 4 texels, 16 lanes per
//                      block with the block's statistics by xor-shuffles
//   k_packet_decode<MODE, CODED>  CODED fetches every texel through fetch_texel, which decodes one texel from its 8-byte block
//
//   k_packet_depth_encode  the depth packet ("FVPD"): the same walk over a texel's owned pixels (walk_owned)
//                      reading the G-buffer's prim and position, reduced by the maximum of the pixels' 16-bit codes; a 2-byte
//                      store per texel
//   k_packet_depth_decode  k_packet_decode's search (find_last_texel) with "code != 0" for "alpha != 0"; a float per pixel
//
// The definition in integers is tests/packet_ref.py, of the block code tests/packet_bc_ref.py, of the depth packet
// tests/packet_depth_ref.py.
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

// The walk over the pixels that launch index (lx, ly) of pass p (factor f, offsets offx / offy) OWNS: those of its clamped
// fill x fill block, each once, whose last writer it is (find_last_writer).  own(u, v, px, py): pixel (px, py) is column u, row v
// of the block.  Both encoders' texels are reductions over this walk.
template <class Own>
__device__ __forceinline__ void walk_owned(const FrameDev& fd, int p, uint32_t f, uint32_t fill, uint32_t offx, uint32_t offy, uint32_t lx, uint32_t ly,
                                  Own own)
{
    const uint32_t ix = lx * f + offx, iy = ly * f + offy;            // (uint32: wraps)
    const uint32_t W = (uint32_t)fd.w, H = (uint32_t)fd.h;
#pragma unroll 1
    for (uint32_t v = 0; v < fill; v++) {
        if (seen_before(iy, v, H)) continue;
        const uint32_t py = block_pixel(iy, v, H);
#pragma unroll 1
        for (uint32_t u = 0; u < fill; u++) {
            if (seen_before(ix, u, W)) continue;
            const uint32_t px = block_pixel(ix, u, W);
            int wp = 0;
            uint32_t wlx, wly;
            if (!find_last_writer(fd, px, py, wp, wlx, wly) || wp != p || wlx != lx || wly != ly) continue;
            own(u, v, px, py);
        }
    }
}

// The colour texel of launch index (lx, ly) of pass p: the mean of the pixels it owns, alpha 0xff; 0 where it owns none.  vec:
// `in` is 16-byte aligned and the frame's width a multiple of 4.
__device__ inline uint32_t owned_texel(const FrameDev& fd, const uint32_t* __restrict__ in, uint32_t vec, int p, uint32_t f, uint32_t fill,
                                       uint32_t offx, uint32_t offy, uint32_t lx, uint32_t ly)
{
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
    walk_owned(fd, p, f, fill, offx, offy, lx, ly, [&](uint32_t u, uint32_t v, uint32_t px, uint32_t py) __attribute__((always_inline)) {
        const uint32_t c = rows4 ? (v == 0u ? pick(q0, u) : v == 1u ? pick(q1, u) : v == 2u ? pick(q2, u) : pick(q3, u)) : in[(size_t)py * W + px];
        n++;
        sr += c & 0xffu; sg += (c >> 8) & 0xffu; sb += (c >> 16) & 0xffu;
    });
    uint32_t texel = 0u;
    if (n) {
        const uint32_t h = n >> 1;
        texel = ((sr + h) / n) | (((sg + h) / n) << 8) | (((sb + h) / n) << 16) | 0xff000000u;
    }
    return texel;
}

// the header from the argument struct, word by word
__device__ inline void store_header(const fovpt_packet_header& h, uint32_t* __restrict__ out)
{
    out[0] = h.magic; out[1] = h.version; out[2] = h.bytes; out[3] = h.sequence;
    out[4] = (uint32_t)h.width; out[5] = (uint32_t)h.height; out[6] = h.npass; out[7] = h._reserved;
#pragma unroll
    for (int p = 0; p < FOVPT_MAX_PASSES; p++) {
        const fovpt_packet_pass& P = h.pass[p];
        uint32_t* o = out + 8 + 8 * p;
        o[0] = P.gw; o[1] = P.gh; o[2] = P.factor; o[3] = P.fill; o[4] = P.offx; o[5] = P.offy; o[6] = P.texels; o[7] = P._reserved;
    }
}

__global__ __launch_bounds__(FOVPT_BLOCK) void k_packet_encode(const FrameDev fd, const PacketArgs a, const uint32_t* __restrict__ in,
                                                               uint32_t* __restrict__ out, uint32_t vec)
{
    const uint32_t t = blockIdx.x * FOVPT_BLOCK + threadIdx.x;
    if (t == 0u) store_header(a.h, out);
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
    out[FOVPT_PACKET_HEADER_BYTES / 4u + t] = owned_texel(fd, in, vec, p, f, fill, offx, offy, lx, ly);
}

// ---- the BC1 block code (the definition in integers: tests/packet_bc_ref.py) -------------------------------------------------------
__device__ inline uint32_t q5(uint32_t c) { return (31u * c + 127u) / 255u; }
__device__ inline uint32_t q6(uint32_t c) { return (63u * c + 127u) / 255u; }
__device__ inline uint32_t pack565(uint32_t r, uint32_t g, uint32_t b) { return q5(r) << 11 | q6(g) << 5 | q5(b); }
// a 565 colour expanded to r | g << 8 | b << 16
__device__ inline uint32_t expand565(uint32_t c)
{
    const uint32_t r = c >> 11, g = (c >> 5) & 63u, b = c & 31u;
    return (r << 3 | r >> 2) | (g << 2 | g >> 4) << 8 | (b << 3 | b >> 2) << 16;
}
// per byte of the low three: a op b
__device__ inline uint32_t min3x8(uint32_t a, uint32_t b)
{
    return min(a & 0xffu, b & 0xffu) | min(a & 0xff00u, b & 0xff00u) | min(a & 0xff0000u, b & 0xff0000u);
}
__device__ inline uint32_t max3x8(uint32_t a, uint32_t b)
{
    return max(a & 0xffu, b & 0xffu) | max(a & 0xff00u, b & 0xff00u) | max(a & 0xff0000u, b & 0xff0000u);
}
// palette entry j of a block with endpoints P0, P1 (expanded), four: color0 > color1; r | g << 8 | b << 16
__device__ inline uint32_t palette(uint32_t P0, uint32_t P1, bool four, uint32_t j)
{
    if (j == 0u) return P0;
    if (j == 1u) return P1;
    uint32_t o = 0u;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint32_t x = (P0 >> (8 * k)) & 0xffu, y = (P1 >> (8 * k)) & 0xffu;
        const uint32_t v = four ? (j == 2u ? (2u * x + y + 1u) / 3u : (x + 2u * y + 1u) / 3u) : (x + y + 1u) >> 1;
        o |= v << (8 * k);
    }
    return o;
}
__device__ inline uint32_t dist2(uint32_t c, uint32_t q)
{
    uint32_t d = 0u;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int e = (int)((c >> (8 * k)) & 0xffu) - (int)((q >> (8 * k)) & 0xffu);
        d += (uint32_t)(e * e);
    }
    return d;
}
// One texel of a BC1 pass: block by * bw + bx at blocks, 8 bytes each (4-byte aligned).
__device__ inline uint32_t bc1_texel(const uint32_t* __restrict__ blocks, uint32_t gw, uint32_t lx, uint32_t ly)
{
    const uint32_t bw = (gw + 3u) >> 2;
    const uint32_t* b = blocks + 2u * ((size_t)(ly >> 2) * bw + (lx >> 2));
    const uint32_t cc = b[0], c0 = cc & 0xffffu, c1 = cc >> 16;
    const uint32_t j = (b[1] >> (2u * (4u * (ly & 3u) + (lx & 3u)))) & 3u;
    const bool four = c0 > c1;
    if (j == 3u && !four) return 0u;
    return 0xff000000u | palette(expand565(c0), expand565(c1), four, j);
}

// All passes of a coded packet in one launch (a.first[p]: the first thread of pass p, a multiple of 16; pass._reserved: the
// codec).  A raw pass takes one thread per texel.  A BC1 pass takes 16 consecutive lanes per block, lane j texel (4 bx + (j & 3),
// 4 by + (j >> 2)): each computes its texel with owned_texel, the block's statistics are xor-shuffles within the 16 lanes, and
// lane 0 stores the 8 bytes.  Every lane of a group reaches every shuffle.  No LDS, no atomics.
__global__ __launch_bounds__(FOVPT_BLOCK) void k_packet_encode_coded(const FrameDev fd, const PacketArgs a, const uint32_t* __restrict__ in,
                                                                     uint32_t* __restrict__ out, uint32_t vec)
{
    const uint32_t t = blockIdx.x * FOVPT_BLOCK + threadIdx.x;
    if (t == 0u) store_header(a.h, out);
    if (t >= a.first[FOVPT_MAX_PASSES]) return;                       // (a multiple of 16: whole groups leave)
    const int p = t < a.first[1] ? 0 : t < a.first[2] ? 1 : 2;
    const fovpt_packet_pass& P0 = a.h.pass[0];
    const fovpt_packet_pass& P1 = a.h.pass[1];
    const fovpt_packet_pass& P2 = a.h.pass[2];
    const uint32_t gw = p == 0 ? P0.gw : p == 1 ? P1.gw : P2.gw, gh = p == 0 ? P0.gh : p == 1 ? P1.gh : P2.gh;
    const uint32_t f = p == 0 ? P0.factor : p == 1 ? P1.factor : P2.factor, fill = p == 0 ? P0.fill : p == 1 ? P1.fill : P2.fill;
    const uint32_t offx = p == 0 ? P0.offx : p == 1 ? P1.offx : P2.offx, offy = p == 0 ? P0.offy : p == 1 ? P1.offy : P2.offy;
    const uint32_t codec = p == 0 ? P0._reserved : p == 1 ? P1._reserved : P2._reserved;
    uint32_t* dst = out + ((p == 0 ? P0.texels : p == 1 ? P1.texels : P2.texels) >> 2);
    const uint32_t li = t - (p == 0 ? a.first[0] : p == 1 ? a.first[1] : a.first[2]);
    if (codec == FOVPT_PACKET_RAW) {
        if (li >= gw * gh) return;                                    // (the pass's threads are rounded up to 16)
        const uint32_t ly = li / gw, lx = li - ly * gw;
        dst[li] = owned_texel(fd, in, vec, p, f, fill, offx, offy, lx, ly);
        return;
    }
    const uint32_t bw = (gw + 3u) >> 2, blk = li >> 4, j = li & 15u;
    const uint32_t by = blk / bw, bx = blk - by * bw;
    const uint32_t lx = 4u * bx + (j & 3u), ly = 4u * by + (j >> 2);
    const uint32_t c = lx < gw && ly < gh ? owned_texel(fd, in, vec, p, f, fill, offx, offy, lx, ly) : 0u;
    const bool live = (c >> 24) != 0u;
    const uint32_t rgb = c & 0xffffffu;
    const uint32_t mask = (uint32_t)(__ballot(live) >> (threadIdx.x & 48u)) & 0xffffu;      // the group's live lanes
    uint32_t lo = live ? rgb : 0xffffffu, hi = live ? rgb : 0u;
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
        lo = min3x8(lo, (uint32_t)__shfl_xor((int)lo, m, 16));
        hi = max3x8(hi, (uint32_t)__shfl_xor((int)hi, m, 16));
    }
    const int lr = (int)(lo & 0xffu), lg = (int)((lo >> 8) & 0xffu), lb = (int)(lo >> 16);
    const int hr = (int)(hi & 0xffu), hg = (int)((hi >> 8) & 0xffu), hb = (int)(hi >> 16);
    const int er = hr - lr, eg = hg - lg, eb = hb - lb;
    const int ref = eg >= er && eg >= eb ? 1 : er >= eb ? 0 : 2;      // ties: g, then r, then b
    // the two other channels, k1 < k2
    const int dr = live ? 2 * (int)(rgb & 0xffu) - lr - hr : 0, dg = live ? 2 * (int)((rgb >> 8) & 0xffu) - lg - hg : 0;
    const int db = live ? 2 * (int)(rgb >> 16) - lb - hb : 0;
    const int dref = ref == 1 ? dg : ref == 0 ? dr : db;
    int s1 = (ref == 0 ? dg : dr) * dref, s2 = (ref == 2 ? dg : db) * dref;
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
        s1 += __shfl_xor(s1, m, 16);
        s2 += __shfl_xor(s2, m, 16);
    }
    // endpoint A takes the reference channel's hi; another channel's hi unless it falls while the reference rises
    const bool f1 = s1 < 0, f2 = s2 < 0;
    const bool fr = ref == 0 ? false : f1, fg = ref == 1 ? false : ref == 0 ? f1 : f2, fb = ref == 2 ? false : f2;
    const uint32_t ea = pack565((uint32_t)(fr ? lr : hr), (uint32_t)(fg ? lg : hg), (uint32_t)(fb ? lb : hb));
    const uint32_t eb565 = pack565((uint32_t)(fr ? hr : lr), (uint32_t)(fg ? hg : lg), (uint32_t)(fb ? hb : lb));
    const bool four = ea != eb565 && mask == 0xffffu;
    const uint32_t c0 = four ? max(ea, eb565) : min(ea, eb565), c1 = four ? min(ea, eb565) : max(ea, eb565);
    const uint32_t E0 = expand565(c0), E1 = expand565(c1);
    uint32_t idx = 3u;
    if (live) {
        uint32_t best = dist2(rgb, E0);
        idx = 0u;
        const uint32_t n = four ? 4u : 3u;
#pragma unroll
        for (uint32_t k = 1; k < 4; k++) {
            const uint32_t d = dist2(rgb, palette(E0, E1, four, k));
            if (k < n && d < best) { best = d; idx = k; }
        }
    }
    uint32_t bits = idx << (2u * j);
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) bits |= (uint32_t)__shfl_xor((int)bits, m, 16);
    if (j == 0u) {
        dst[2u * blk] = mask ? c0 | c1 << 16 : 0u;
        dst[2u * blk + 1u] = mask ? bits : 0xffffffffu;
    }
}

// The last texel whose block reaches pixel (x, y) and whose alpha is not 0, in the definition's write order: the highest pass,
// within it the launch index that comes last.  find_last_writer's search (fovpt_pixel.h) over the header's pass records.
// texel (lx, ly) of a pass whose array starts at tex: as stored, or decoded from its BC1 block (a coded packet: pass._reserved is the codec)
template <bool CODED>
__device__ inline uint32_t fetch_texel(const uint32_t* __restrict__ tex, const fovpt_packet_pass& P, uint32_t lx, uint32_t ly)
{
    if (CODED && P._reserved == FOVPT_PACKET_BC1) return bc1_texel(tex, P.gw, lx, ly);
    return tex[(size_t)ly * P.gw + lx];
}

// fetch(P, lx, ly, val): texel (lx, ly) of pass P into val, true where it is live (a colour texel: alpha != 0; a depth code: != 0)
template <class Fetch>
__device__ inline bool find_last_texel(const fovpt_packet_header& h, uint32_t x, uint32_t y, int& wp, uint32_t& wlx, uint32_t& wly, uint32_t& val,
                                       Fetch fetch)
{
    const uint32_t W = (uint32_t)h.width, H = (uint32_t)h.height;
#pragma unroll
    for (int p = FOVPT_MAX_PASSES - 1; p >= 0; p--) {
        if ((uint32_t)p >= h.npass) continue;
        const fovpt_packet_pass& P = h.pass[p];
        const uint32_t f = P.factor;
        // blocks that tile the plane, away from the last column and row: one candidate per axis
        if (P.fill == f && (f & (f - 1u)) == 0u && x + 1u != W && y + 1u != H) {
            const int sh = 31 - __clz((int)f);
            const long long rx = (long long)x - (long long)(int32_t)P.offx, ry = (long long)y - (long long)(int32_t)P.offy;
            if (rx < 0 || ry < 0 || rx >= ((long long)P.gw << sh) || ry >= ((long long)P.gh << sh)) continue;
            const uint32_t lx = (uint32_t)rx >> sh, ly = (uint32_t)ry >> sh;
            uint32_t c;
            if (!fetch(P, lx, ly, c)) continue;
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
                uint32_t c;
                if (!fetch(P, (uint32_t)lx, (uint32_t)ly, c)) continue;
                wp = p; wlx = (uint32_t)lx; wly = (uint32_t)ly; val = c;
                return true;
            }
        }
    }
    return false;
}

template <int MODE, bool CODED>
__global__ __launch_bounds__(FOVPT_BLOCK) void k_packet_decode(const PacketArgs a, const uint32_t* __restrict__ pk, uint32_t* __restrict__ out)
{
    const uint32_t W = (uint32_t)a.h.width, H = (uint32_t)a.h.height;
    const uint32_t idx = blockIdx.x * FOVPT_BLOCK + threadIdx.x;      // (W * H <= 2^28)
    if (idx >= W * H) return;
    const uint32_t y = idx / W, x = idx - y * W;
    int p = 0;
    uint32_t lx, ly, val;
    const auto fetch = [pk](const fovpt_packet_pass& P, uint32_t tx, uint32_t ty, uint32_t& c) {
        c = fetch_texel<CODED>(pk + (P.texels >> 2), P, tx, ty);
        return (c >> 24) != 0u;
    };
    if (!find_last_texel(a.h, x, y, p, lx, ly, val, fetch)) return;          // (no texel reaches the pixel: it keeps what it held)
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
            uint32_t cx, cy, cd;
            if (CODED) {
                const fovpt_packet_pass& P = p == 0 ? P0 : p == 1 ? P1 : P2;
                cx = inx ? fetch_texel<CODED>(tex, P, (uint32_t)tx, ly) : 0u;
                cy = iny ? fetch_texel<CODED>(tex, P, lx, (uint32_t)ty) : 0u;
                cd = inx && iny ? fetch_texel<CODED>(tex, P, (uint32_t)tx, (uint32_t)ty) : 0u;
            } else {
                cx = inx ? tex[(size_t)ly * gw + (size_t)tx] : 0u;
                cy = iny ? tex[(size_t)ty * gw + lx] : 0u;
                cd = inx && iny ? tex[(size_t)ty * gw + (size_t)tx] : 0u;
            }
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

// ---- the depth packet ("FVPD"; the definition: tests/packet_depth_ref.py) ------------------------------------
// The code of G-buffer entry (prim, X): 1 for the sky and for a point not in front of the camera, else 2 .. 65535, linear in
// near / z with z the point's depth along W (m2: the third row of the rendered camera's inverse).
__device__ inline uint32_t depth_code(uint32_t prim, const float4& X, const float* eye, const float* m2, float near)
{
    if (prim == 0xffffffffu) return 1u;
    const V3 v = v3(X) - v3(eye[0], eye[1], eye[2]);
    const float z = (m2[0] * v.x + m2[1] * v.y) + m2[2] * v.z;
    if (!(z > 0.0f) || !(z < INFINITY)) return 1u;                    // (NaN fails the first)
    const float q = near / z;
    const float c = fmaxf(1.0f, fminf(floorf(q * 65534.0f + 0.5f), 65534.0f));
    return (uint32_t)c + 1u;
}

// One thread per texel of all passes: the largest code of the pixels it owns (walk_owned), 0 where it owns none, stored as its
// own 2 bytes; the thread of an odd pass's last texel stores the 2 bytes of padding behind it, and thread 0 the 48 header words.
__global__ __launch_bounds__(FOVPT_BLOCK) void k_packet_depth_encode(const FrameDev fd, const PacketDepthArgs a, const uint32_t* __restrict__ prim,
                                                                     const float4* __restrict__ pos, uint32_t* __restrict__ out)
{
    const uint32_t t = blockIdx.x * FOVPT_BLOCK + threadIdx.x;
    if (t == 0u) {
        store_header(a.h.base, out);
        const float* cam = &a.h.camera.eye.x;
#pragma unroll
        for (int k = 0; k < 12; k++) out[32 + k] = __float_as_uint(cam[k]);
        out[44] = __float_as_uint(a.h.near); out[45] = a.h._reserved[0]; out[46] = a.h._reserved[1]; out[47] = a.h._reserved[2];
    }
    if (t >= a.first[FOVPT_MAX_PASSES]) return;
    const int p = t < a.first[1] ? 0 : t < a.first[2] ? 1 : 2;
    const fovpt_packet_pass& P0 = a.h.base.pass[0];
    const fovpt_packet_pass& P1 = a.h.base.pass[1];
    const fovpt_packet_pass& P2 = a.h.base.pass[2];
    const uint32_t gw = p == 0 ? P0.gw : p == 1 ? P1.gw : P2.gw, gh = p == 0 ? P0.gh : p == 1 ? P1.gh : P2.gh;
    const uint32_t f = p == 0 ? P0.factor : p == 1 ? P1.factor : P2.factor, fill = p == 0 ? P0.fill : p == 1 ? P1.fill : P2.fill;
    const uint32_t offx = p == 0 ? P0.offx : p == 1 ? P1.offx : P2.offx, offy = p == 0 ? P0.offy : p == 1 ? P1.offy : P2.offy;
    uint16_t* dst = (uint16_t*)(out + ((p == 0 ? P0.texels : p == 1 ? P1.texels : P2.texels) >> 2));
    const uint32_t li = t - (p == 0 ? a.first[0] : p == 1 ? a.first[1] : a.first[2]);
    const uint32_t ly = li / gw, lx = li - ly * gw;
    const uint32_t W = (uint32_t)fd.w;
    const float* eye = &a.h.camera.eye.x;
    uint32_t code = 0u;
    walk_owned(fd, p, f, fill, offx, offy, lx, ly, [&](uint32_t, uint32_t, uint32_t px, uint32_t py) __attribute__((always_inline)) {
        const size_t s = (size_t)py * W + px;
        code = max(code, depth_code(prim[s], pos[s], eye, a.m2, a.h.near));
    });
    dst[li] = (uint16_t)code;
    const uint32_t n = gw * gh;                                       // (<= 2^26)
    if (li + 1u == n && (n & 1u)) dst[n] = 0;                         // the padding to a multiple of 4
}

__global__ __launch_bounds__(FOVPT_BLOCK) void k_packet_depth_decode(const PacketDepthArgs a, const uint32_t* __restrict__ pk, float* __restrict__ out)
{
    const fovpt_packet_header& h = a.h.base;
    const uint32_t W = (uint32_t)h.width, H = (uint32_t)h.height;
    const uint32_t idx = blockIdx.x * FOVPT_BLOCK + threadIdx.x;      // (W * H <= 2^28)
    if (idx >= W * H) return;
    const uint32_t y = idx / W, x = idx - y * W;
    int p = 0;
    uint32_t lx, ly, code;
    const auto fetch = [pk](const fovpt_packet_pass& P, uint32_t tx, uint32_t ty, uint32_t& c) {
        c = ((const uint16_t*)(pk + (P.texels >> 2)))[(size_t)ty * P.gw + tx];
        return c != 0u;
    };
    if (!find_last_texel(h, x, y, p, lx, ly, code, fetch)) return;    // (no texel reaches the pixel: it keeps what it held)
    out[idx] = code == 1u ? INFINITY : (a.h.near * 65534.0f) / (float)(code - 1u);
}

}  // namespace

void fovpt_launch_packet_depth_encode(hipStream_t st, const FrameDev& fd, const PacketDepthArgs& a, const uint32_t* prim, const float4* pos,
                                      uint32_t* out)
{
    const uint32_t total = a.first[FOVPT_MAX_PASSES];                 // (>= 1: every pass has a launch index)
    hipLaunchKernelGGL(k_packet_depth_encode, dim3((total + FOVPT_BLOCK - 1) / FOVPT_BLOCK), dim3(FOVPT_BLOCK), 0, st, fd, a, prim, pos, out);
}

void fovpt_launch_packet_depth_decode(hipStream_t st, const PacketDepthArgs& a, const uint32_t* packet, float* out)
{
    const uint32_t npix = (uint32_t)a.h.base.width * (uint32_t)a.h.base.height;
    hipLaunchKernelGGL(k_packet_depth_decode, dim3((npix + FOVPT_BLOCK - 1) / FOVPT_BLOCK), dim3(FOVPT_BLOCK), 0, st, a, packet, out);
}

void fovpt_launch_packet_encode(hipStream_t st, const FrameDev& fd, const PacketArgs& a, const uint32_t* in, uint32_t* out)
{
    const uint32_t total = a.first[FOVPT_MAX_PASSES];                 // (>= 1: every pass has a launch index)
    const uint32_t vec = ((uintptr_t)in & 15u) == 0u && (fd.w & 3) == 0 ? 1u : 0u;
    hipLaunchKernelGGL(k_packet_encode, dim3((total + FOVPT_BLOCK - 1) / FOVPT_BLOCK), dim3(FOVPT_BLOCK), 0, st, fd, a, in, out, vec);
}

// a.first[]: the first thread of each pass and their total (packet_args of api_packet.hip)
void fovpt_launch_packet_encode_coded(hipStream_t st, const FrameDev& fd, const PacketArgs& a, const uint32_t* in, uint32_t* out)
{
    const uint32_t total = a.first[FOVPT_MAX_PASSES];
    const uint32_t vec = ((uintptr_t)in & 15u) == 0u && (fd.w & 3) == 0 ? 1u : 0u;
    hipLaunchKernelGGL(k_packet_encode_coded, dim3((total + FOVPT_BLOCK - 1) / FOVPT_BLOCK), dim3(FOVPT_BLOCK), 0, st, fd, a, in, out, vec);
}

void fovpt_launch_packet_decode(hipStream_t st, const PacketArgs& a, int mode, const uint32_t* packet, uint32_t* out)
{
    const uint32_t npix = (uint32_t)a.h.width * (uint32_t)a.h.height;
    const dim3 grid((npix + FOVPT_BLOCK - 1) / FOVPT_BLOCK), block(FOVPT_BLOCK);
    const bool smooth = mode == FOVPT_PACKET_SMOOTH;
    if (a.h.magic == FOVPT_PACKET_MAGIC_CODED) {
        if (smooth) hipLaunchKernelGGL((k_packet_decode<FOVPT_PACKET_SMOOTH, true>), grid, block, 0, st, a, packet, out);
        else hipLaunchKernelGGL((k_packet_decode<FOVPT_PACKET_NEAREST, true>), grid, block, 0, st, a, packet, out);
    } else if (smooth) hipLaunchKernelGGL((k_packet_decode<FOVPT_PACKET_SMOOTH, false>), grid, block, 0, st, a, packet, out);
    else hipLaunchKernelGGL((k_packet_decode<FOVPT_PACKET_NEAREST, false>), grid, block, 0, st, a, packet, out);
}
