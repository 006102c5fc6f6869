// packet_host.cpp -- the foveated frame packet for a client: fovpt_packet_check and fovpt_packet_decode_host (include/fovpt.h;
// the definition in integers: tests/packet_ref.py, of a coded packet's BC1 passes tests/packet_bc_ref.py).  Host-only C++ without a context, for untrusted bytes: compiled into
// libfovpt.so and into libfovpt_loader.so, the library for machines without ROCm.  Every read goes through memcpy inside
// [packet, packet + header.bytes), which the checks have shown to lie inside the caller's bytes; every write is to a pixel
// index clamped into the output.  The depth packet ("FVPD": fovpt_packet_depth_defaults, fovpt_packet_check_depth and
// fovpt_packet_decode_depth_host; the definition: tests/packet_depth_ref.py) shares the checks of the first 128 bytes.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "fovpt_camera.h"
#include "fovpt_packet.h"

void fovpt_internal_set_error(const char* text);      // fovpt_api.hip / loader_host.cpp: the text fovpt_last_error(NULL) returns

static_assert(sizeof(fovpt_packet_header) == FOVPT_PACKET_HEADER_BYTES, "packet header");

static_assert(sizeof(fovpt_packet_depth_header) == FOVPT_PACKET_DEPTH_HEADER_BYTES, "depth packet header");

namespace {

// The checks on the 128 bytes every kind of packet starts with.  depth: an "FVPD" packet -- the arrays start behind 192 bytes
// and hold 2 bytes per texel, padded to 4; otherwise "FVPK" or "FVPC" by the magic.
const char* common_header_error(const fovpt_packet_header* h, uint64_t avail, bool depth)
{
    const bool coded = !depth && h->magic == FOVPT_PACKET_MAGIC_CODED;   // ("FVPC": the pass's eighth word is its codec)
    const uint32_t head = depth ? FOVPT_PACKET_DEPTH_HEADER_BYTES : FOVPT_PACKET_HEADER_BYTES;
    if (depth ? h->magic != FOVPT_PACKET_MAGIC_DEPTH : h->magic != FOVPT_PACKET_MAGIC && !coded) return "wrong magic";
    if (h->version != FOVPT_PACKET_VERSION) return "unknown version";
    if (h->bytes > avail || h->bytes < head) return depth ? "bytes field outside 192 .. the bytes given" : "bytes field outside 128 .. the bytes given";
    if (h->width < 1 || h->width > FOVPT_PACKET_MAX_DIM || h->height < 1 || h->height > FOVPT_PACKET_MAX_DIM) return "width / height outside 1 .. 16384";
    if (h->npass < 1 || h->npass > 3) return "npass outside 1 .. 3";
    if (h->_reserved) return "non-zero reserved field";
    uint64_t texels = 0;
    for (uint32_t p = 0; p < 3; p++) {
        const fovpt_packet_pass& P = h->pass[p];
        if (p >= h->npass) {
            if (P.gw | P.gh | P.factor | P.fill | P.offx | P.offy | P.texels | P._reserved) return "non-zero unused pass entry";
            continue;
        }
        if (coded ? P._reserved > FOVPT_PACKET_BC1 : P._reserved != 0u) return coded ? "unknown codec" : "non-zero reserved field";
        if (P.gw == 0 || P.gh == 0) return "empty launch grid";
        const uint64_t n = (uint64_t)P.gw * (uint64_t)P.gh;               // (< 2^64)
        if (n > FOVPT_PACKET_MAX_TEXELS || (texels += n) > FOVPT_PACKET_MAX_TEXELS) return "more than 2^26 texels";
        if (P.factor == 0) return "factor 0";
        if (P.fill < 1 || P.fill > FOVPT_PACKET_MAX_FILL) return "fill outside 1 .. 8";
        if (P.texels < head || (P.texels & 3u)) return depth ? "code offset below 192 or not a multiple of 4" : "texel offset below 128 or not a multiple of 4";
        const uint64_t size = depth ? fovpt_packet_depth_pass_bytes(P.gw, P.gh) : fovpt_packet_pass_bytes(P.gw, P.gh, P._reserved);
        if ((uint64_t)P.texels + size > (uint64_t)h->bytes) return "texel array outside the packet";
    }
    return nullptr;
}

}  // namespace

const char* fovpt_packet_header_error(const fovpt_packet_header* h, uint64_t avail) { return common_header_error(h, avail, false); }

const char* fovpt_packet_depth_header_error(const fovpt_packet_depth_header* h, uint64_t avail)
{
    if (const char* why = common_header_error(&h->base, avail, true)) return why;
    const float* cam = &h->camera.eye.x;                                 // eye, U, V, W: 12 floats
    for (int k = 0; k < 12; k++)
        if (!std::isfinite(cam[k])) return "non-finite camera entry";
    float inv[9];
    if (!fovpt_camera_inverse(&h->camera.U.x, &h->camera.V.x, &h->camera.W.x, inv)) return "singular camera";
    if (!(std::isfinite(h->near) && h->near > 0.0f)) return "near is not finite and above 0";
    if (h->_reserved[0] | h->_reserved[1] | h->_reserved[2]) return "non-zero reserved field";
    return nullptr;
}

namespace {

int refuse(const char* who, const char* why)
{
    char buf[160];
    snprintf(buf, sizeof(buf), "%s: %s", who, why);
    fovpt_internal_set_error(buf);
    return FOVPT_E_INVALID;
}

int read_header(const char* who, const void* packet, size_t bytes, fovpt_packet_header& h)
{
    if (!packet) return refuse(who, "null packet");
    if (bytes < FOVPT_PACKET_HEADER_BYTES) return refuse(who, "fewer than 128 bytes");
    memcpy(&h, packet, sizeof(h));
    if (const char* why = fovpt_packet_header_error(&h, (uint64_t)bytes)) return refuse(who, why);
    return FOVPT_OK;
}

int read_depth_header(const char* who, const void* packet, size_t bytes, fovpt_packet_depth_header& h)
{
    if (!packet) return refuse(who, "null packet");
    if (bytes < FOVPT_PACKET_DEPTH_HEADER_BYTES) return refuse(who, "fewer than 192 bytes");
    memcpy(&h, packet, sizeof(h));
    if (const char* why = fovpt_packet_depth_header_error(&h, (uint64_t)bytes)) return refuse(who, why);
    return FOVPT_OK;
}

// one texel of a BC1 pass, decoded from its 8-byte block (include/fovpt.h; tests/packet_bc_ref.py)
inline uint32_t bc1_texel(const unsigned char* blocks, uint32_t gw, uint32_t lx, uint32_t ly)
{
    const uint64_t bw = ((uint64_t)gw + 3u) >> 2;
    uint32_t w[2];
    memcpy(w, blocks + 8ull * ((uint64_t)(ly >> 2) * bw + (lx >> 2)), 8);
    const uint32_t c0 = w[0] & 0xffffu, c1 = w[0] >> 16, j = (w[1] >> (2u * (4u * (ly & 3u) + (lx & 3u)))) & 3u;
    const bool four = c0 > c1;
    if (j == 3u && !four) return 0u;
    const uint32_t e0[3] = {c0 >> 11, (c0 >> 5) & 63u, c0 & 31u}, e1[3] = {c1 >> 11, (c1 >> 5) & 63u, c1 & 31u};
    uint32_t v = 0xff000000u;
    for (int k = 0; k < 3; k++) {
        const uint32_t x = k == 1 ? (e0[k] << 2 | e0[k] >> 4) : (e0[k] << 3 | e0[k] >> 2), y = k == 1 ? (e1[k] << 2 | e1[k] >> 4) : (e1[k] << 3 | e1[k] >> 2);
        const uint32_t c = j == 0u ? x : j == 1u ? y : !four ? (x + y + 1u) / 2u : j == 2u ? (2u * x + y + 1u) / 3u : (x + 2u * y + 1u) / 3u;
        v |= c << (8 * k);
    }
    return v;
}

// (an "FVPK" pass has _reserved 0 = FOVPT_PACKET_RAW)
inline uint32_t texel(const unsigned char* base, const fovpt_packet_pass& P, uint32_t lx, uint32_t ly)
{
    if (P._reserved == FOVPT_PACKET_BC1) return bc1_texel(base + P.texels, P.gw, lx, ly);
    uint32_t v;
    memcpy(&v, base + P.texels + 4ull * ((uint64_t)ly * P.gw + lx), 4);
    return v;
}

inline uint32_t clamp_pixel(uint32_t i, uint32_t dim) { return i < dim ? i : dim - 1u; }

}  // namespace

extern "C" {

int fovpt_packet_check(const void* packet, size_t bytes)
{
    fovpt_packet_header h;
    return read_header("fovpt_packet_check", packet, bytes, h);
}

int fovpt_packet_decode_host(const void* packet, size_t bytes, int mode, uint32_t* out_rgba, int width, int height)
{
    const char* who = "fovpt_packet_decode_host";
    fovpt_packet_header h;
    { const int rc_ = read_header(who, packet, bytes, h); if (rc_) return rc_; }
    if (mode != FOVPT_PACKET_NEAREST && mode != FOVPT_PACKET_SMOOTH) return refuse(who, "unknown mode");
    if (!out_rgba) return refuse(who, "null output");
    if (width != h.width || height != h.height) return refuse(who, "the output's size differs from the packet's");
    const unsigned char* base = (const unsigned char*)packet;
    const uint32_t W = (uint32_t)h.width, H = (uint32_t)h.height;
    // SMOOTH: which texel wrote each pixel last (pass << 26 | launch index; a packet holds at most 2^26 texels), 0xffffffff: none
    std::vector<uint32_t> owner;
    if (mode == FOVPT_PACKET_SMOOTH) {
        try { owner.assign((size_t)W * H, 0xffffffffu); } catch (const std::bad_alloc&) {
            fovpt_internal_set_error("fovpt_packet_decode_host: out of memory");
            return FOVPT_E_NOMEM;
        }
    }
    // the forward loop of the definition: pass order, ascending (ly, lx), later writes win
    for (uint32_t p = 0; p < h.npass; p++) {
        const fovpt_packet_pass& P = h.pass[p];
        for (uint32_t ly = 0; ly < P.gh; ly++)
            for (uint32_t lx = 0; lx < P.gw; lx++) {
                const uint32_t t = texel(base, P, lx, ly);
                if (!(t >> 24)) continue;
                const uint32_t ix = lx * P.factor + P.offx, iy = ly * P.factor + P.offy;      // (uint32: wraps)
                for (uint32_t v = 0; v < P.fill; v++) {
                    const size_t row = (size_t)clamp_pixel(iy + v, H) * W;
                    for (uint32_t u = 0; u < P.fill; u++) {
                        const size_t at = row + clamp_pixel(ix + u, W);
                        out_rgba[at] = t;
                        if (mode == FOVPT_PACKET_SMOOTH) owner[at] = (p << 26) | (ly * P.gw + lx);
                    }
                }
            }
    }
    if (mode != FOVPT_PACKET_SMOOTH) return FOVPT_OK;
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++) {
            const uint32_t o = owner[(size_t)y * W + x];
            if (o == 0xffffffffu) continue;
            const fovpt_packet_pass& P = h.pass[o >> 26];
            const uint32_t li = o & 0x3ffffffu, fill = P.fill;
            if (fill != P.factor || fill < 2) continue;
            const uint32_t lx = li % P.gw, ly = li / P.gw;
            const uint32_t ix = lx * P.factor + P.offx, iy = ly * P.factor + P.offy;
            if (x < ix || (uint64_t)x >= (uint64_t)ix + fill || y < iy || (uint64_t)y >= (uint64_t)iy + fill) continue;      // not regular
            const int dx = 2 * (int)(x - ix) + 1 - (int)fill, dy = 2 * (int)(y - iy) + 1 - (int)fill;
            const int sx = dx > 0 ? 1 : -1, sy = dy > 0 ? 1 : -1;
            const uint32_t adx = (uint32_t)(dx < 0 ? -dx : dx), ady = (uint32_t)(dy < 0 ? -dy : dy);
            const uint32_t wx[2] = {2 * fill - adx, adx}, wy[2] = {2 * fill - ady, ady};
            uint32_t sum[3] = {0, 0, 0}, total = 0;
            for (int j = 0; j < 2; j++)
                for (int i = 0; i < 2; i++) {
                    const int64_t tx = (int64_t)lx + i * sx, ty = (int64_t)ly + j * sy;
                    if (tx < 0 || tx >= (int64_t)P.gw || ty < 0 || ty >= (int64_t)P.gh) continue;
                    const uint32_t c = texel(base, P, (uint32_t)tx, (uint32_t)ty);
                    if (!(c >> 24)) continue;
                    const uint32_t wt = wx[i] * wy[j];
                    total += wt;
                    for (int k = 0; k < 3; k++) sum[k] += wt * ((c >> (8 * k)) & 0xffu);
                }
            uint32_t v = 0xff000000u;
            for (int k = 0; k < 3; k++) v |= ((sum[k] + total / 2) / total) << (8 * k);
            out_rgba[(size_t)y * W + x] = v;
        }
    return FOVPT_OK;
}

// ---- the depth packet ("FVPD"; the definition: tests/packet_depth_ref.py) ------------------------------------------------------
// (near: a convention, not a measurement: include/fovpt.h)
void fovpt_packet_depth_defaults(fovpt_packet_depth_config* cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->near = 0.1f;
}

int fovpt_packet_check_depth(const void* packet, size_t bytes)
{
    fovpt_packet_depth_header h;
    return read_depth_header("fovpt_packet_check_depth", packet, bytes, h);
}

int fovpt_packet_decode_depth_host(const void* packet, size_t bytes, float* out_depth, int width, int height)
{
    const char* who = "fovpt_packet_decode_depth_host";
    fovpt_packet_depth_header h;
    { const int rc_ = read_depth_header(who, packet, bytes, h); if (rc_) return rc_; }
    if (!out_depth) return refuse(who, "null output");
    if (width != h.base.width || height != h.base.height) return refuse(who, "the output's size differs from the packet's");
    const unsigned char* base = (const unsigned char*)packet;
    const uint32_t W = (uint32_t)h.base.width, H = (uint32_t)h.base.height;
    const float scale = h.near * 65534.0f;
    // the forward loop of the definition: pass order, ascending (ly, lx), later writes win
    for (uint32_t p = 0; p < h.base.npass; p++) {
        const fovpt_packet_pass& P = h.base.pass[p];
        for (uint32_t ly = 0; ly < P.gh; ly++)
            for (uint32_t lx = 0; lx < P.gw; lx++) {
                uint16_t code;
                memcpy(&code, base + P.texels + 2ull * ((uint64_t)ly * P.gw + lx), 2);
                if (!code) continue;
                const float d = code == 1u ? INFINITY : scale / (float)(code - 1u);
                const uint32_t ix = lx * P.factor + P.offx, iy = ly * P.factor + P.offy;      // (uint32: wraps)
                for (uint32_t v = 0; v < P.fill; v++) {
                    const size_t row = (size_t)clamp_pixel(iy + v, H) * W;
                    for (uint32_t u = 0; u < P.fill; u++) out_depth[row + clamp_pixel(ix + u, W)] = d;
                }
            }
    }
    return FOVPT_OK;
}

}  // extern "C"
