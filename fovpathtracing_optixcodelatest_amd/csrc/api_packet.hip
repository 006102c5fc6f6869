// api_packet.hip -- foveated frame packets, raw and coded, over the C ABI (include/fovpt.h, fovpt_packet_*): the header of the frame as rendered,
// the encoder (packet.hip) on fovpt_stream(), the slots that take a packet to pinned host memory on a copy stream of the
// context's own, and the device decoder.  The decoder for a client and the checks are packet_host.cpp.
#include <cstring>

#include "fovpt_ctx.h"
#include "fovpt_packet.h"

namespace {

// What describe, encode and submit (`who`) ask: a frame was rendered, whole, at lp's size, and its packet is one the decoders
// accept.  Fills the kernels' arguments; nothing is allocated, enqueued or changed.  cfg: null for an "FVPK" packet, else the
// codecs of a coded one, whose a.first[] counts k_packet_encode_coded's threads.
int packet_args(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_packet_config* cfg, uint32_t sequence, const char* who, PacketArgs& a)
{
    CHK(check_rendered_frame(c, lp, who, nullptr, nullptr, 0));
    const FrameDev& fd = c->rendered.frame;
    if (cfg) {
        if (cfg->_reserved) return fail(c, FOVPT_E_INVALID, "%s: non-zero reserved word in the packet config", who);
        for (int p = 0; p < FOVPT_MAX_PASSES; p++) {
            const uint32_t k = cfg->codec[p];
            if (k == FOVPT_PACKET_BY_FILL) continue;
            if (k > FOVPT_PACKET_BC1) return fail(c, FOVPT_E_INVALID, "%s: unknown codec %u for pass %d", who, k, p);
            if (p >= fd.npass && k) return fail(c, FOVPT_E_INVALID, "%s: codec %u for pass %d of a frame of %d", who, k, p, fd.npass);
        }
    }
    memset(&a, 0, sizeof(a));
    fovpt_packet_header& h = a.h;
    h.magic = cfg ? FOVPT_PACKET_MAGIC_CODED : FOVPT_PACKET_MAGIC; h.version = FOVPT_PACKET_VERSION; h.sequence = sequence;
    h.width = fd.w; h.height = fd.h;
    h.npass = (uint32_t)fd.npass;
    uint64_t at = FOVPT_PACKET_HEADER_BYTES, texels = 0, threads = 0;
    for (int p = 0; p < FOVPT_MAX_PASSES; p++) {
        a.first[p] = (uint32_t)(cfg ? threads : texels);
        if (p >= fd.npass) continue;
        const PassDev& P = fd.pass[p];
        const uint64_t n = (uint64_t)P.gw * (uint64_t)P.gh;
        // (a pass without a launch index -- a side below 4, radii that make an empty grid -- has no texel array to describe;
        // fovpt_packet_check refuses gw or gh 0)
        if (n == 0 || P.fx != P.fy || n > FOVPT_PACKET_MAX_TEXELS || (texels += n) > FOVPT_PACKET_MAX_TEXELS)
            return fail(c, FOVPT_E_INVALID, "%s: pass %d of the frame (%u x %u launch indices) does not fit a packet", who, p, P.gw, P.gh);
        fovpt_packet_pass& O = h.pass[p];
        O.gw = P.gw; O.gh = P.gh; O.factor = P.fx; O.fill = (uint32_t)P.fill; O.offx = P.offx; O.offy = P.offy;
        O.texels = (uint32_t)at;
        if (cfg) O._reserved = cfg->codec[p] == FOVPT_PACKET_BY_FILL ? (P.fill > 1 ? FOVPT_PACKET_BC1 : FOVPT_PACKET_RAW) : cfg->codec[p];
        at += fovpt_packet_pass_bytes(P.gw, P.gh, O._reserved);
        // a raw pass: a thread per texel; a BC1 pass: 16 per block; whole groups of 16 (<= 2^26 + 2^15 per pass)
        threads += O._reserved == FOVPT_PACKET_BC1 ? 16ull * (((uint64_t)P.gw + 3u) >> 2) * (((uint64_t)P.gh + 3u) >> 2) : (n + 15u) & ~15ull;
    }
    a.first[FOVPT_MAX_PASSES] = (uint32_t)(cfg ? threads : texels);
    h.bytes = (uint32_t)at;                                           // (<= 128 + 2^28)
    if (const char* why = fovpt_packet_header_error(&h, at)) return fail(c, FOVPT_E_INVALID, "%s: the frame does not fit a packet: %s", who, why);
    return FOVPT_OK;
}

const uint32_t* packet_input(const fovpt_launch_params* lp, const uint32_t* in_rgba) { return in_rgba ? in_rgba : lp->frame.frame_buffer; }

// what fovpt_packet_submit makes on a context's first call
int packet_slots(fovpt_ctx* c)
{
    if (c->pk_stream) return FOVPT_OK;
    hipStream_t st = nullptr;
    HIPCHK(c, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    for (fovpt_ctx::PacketSlot& S : c->pk_slot) {
        hipError_t e = S.ev_encoded ? hipSuccess : hipEventCreateWithFlags(&S.ev_encoded, hipEventDisableTiming);
        if (e == hipSuccess && !S.ev_done) e = hipEventCreateWithFlags(&S.ev_done, hipEventDisableTiming);
        if (e != hipSuccess) {                                        // (the destructor releases what was made)
            (void)hipStreamDestroy(st);
            return fail(c, FOVPT_E_DEVICE, "fovpt_packet_submit: event creation: %s", hipGetErrorString(e));
        }
    }
    c->pk_stream = st;
    return FOVPT_OK;
}

// The three entry points, raw (cfg null) and coded (coded: cfg must not be null).
int packet_describe(const char* who, bool coded, fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_packet_config* cfg, uint32_t sequence,
                    fovpt_packet_header* out)
{
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !out || (coded && !cfg)) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    PacketArgs a;
    CHK(packet_args(c, lp, cfg, sequence, who, a));
    *out = a.h;
    return FOVPT_OK;
}

void launch_encode(fovpt_ctx* c, const PacketArgs& a, const uint32_t* in, uint32_t* out)
{
    if (a.h.magic == FOVPT_PACKET_MAGIC_CODED) fovpt_launch_packet_encode_coded(c->shadow_stream, c->rendered.frame, a, in, out);
    else fovpt_launch_packet_encode(c->shadow_stream, c->rendered.frame, a, in, out);
}

// Enqueued on fovpt_stream() like fovpt_denoise, and ordered like it: behind the frame's resolve, ahead of the next frame's.
int packet_encode(const char* who, bool coded, fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_packet_config* cfg, const uint32_t* in_rgba,
                  uint32_t sequence, void* out_packet)
{
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !out_packet || (coded && !cfg)) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    if (((uintptr_t)out_packet & 3u) != 0u) return fail(c, FOVPT_E_INVALID, "%s: the packet buffer is not 4-byte aligned", who);
    PacketArgs a;
    CHK(packet_args(c, lp, cfg, sequence, who, a));
    const uint32_t* in = packet_input(lp, in_rgba);
    if (!in) return fail(c, FOVPT_E_NO_FRAME, "%s: null frame_buffer", who);
    HIPCHK(c, hipSetDevice(c->device));
    launch_encode(c, a, in, (uint32_t*)out_packet);
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

// The encode into the slot's own device buffer on fovpt_stream(), an event behind it, and on the copy stream -- which waits for
// that event and for nothing else -- the copy into the slot's pinned buffer and the slot's done-event.  The host waits only for
// the previous copy out of the slot it is about to reuse, if that is still running.
int packet_submit(const char* who, bool coded, fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_packet_config* cfg, const uint32_t* in_rgba,
                  uint32_t sequence, int* slot)
{
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !slot || (coded && !cfg)) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    PacketArgs a;
    CHK(packet_args(c, lp, cfg, sequence, who, a));
    const uint32_t* in = packet_input(lp, in_rgba);
    if (!in) return fail(c, FOVPT_E_NO_FRAME, "%s: null frame_buffer", who);
    HIPCHK(c, hipSetDevice(c->device));
    CHK(packet_slots(c));
    const int k = (int)(c->pk_next % FOVPT_PACKET_SLOTS);
    fovpt_ctx::PacketSlot& S = c->pk_slot[k];
    if (S.submitted) HIPCHK(c, hipEventSynchronize(S.ev_done));
    const size_t bytes = a.h.bytes;
    if (S.host_bytes < bytes) {                                       // (the packet's size follows the frame's size and the radii, not the gaze)
        if (S.host) (void)hipHostFree(S.host);
        S.host = nullptr; S.host_bytes = 0; S.submitted = false;
        HIPCHK(c, hipHostMalloc(&S.host, bytes, hipHostMallocDefault));
        S.host_bytes = bytes;
    }
    HIPCHK(c, S.dev.reserve(bytes));
    launch_encode(c, a, in, (uint32_t*)S.dev.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(S.ev_encoded, c->shadow_stream));
    HIPCHK(c, hipStreamWaitEvent(c->pk_stream, S.ev_encoded, 0));
    HIPCHK(c, hipMemcpyAsync(S.host, S.dev.p, bytes, hipMemcpyDeviceToHost, c->pk_stream));
    HIPCHK(c, hipEventRecord(S.ev_done, c->pk_stream));
    S.bytes = bytes;
    S.submitted = true;
    c->pk_next++;
    *slot = k;
    return FOVPT_OK;
}

}  // namespace

extern "C" {

int fovpt_packet_describe(fovpt_ctx* c, const fovpt_launch_params* lp, uint32_t sequence, fovpt_packet_header* out)
{
    return packet_describe("fovpt_packet_describe", false, c, lp, nullptr, sequence, out);
}
int fovpt_packet_encode(fovpt_ctx* c, const fovpt_launch_params* lp, const uint32_t* in_rgba, uint32_t sequence, void* out_packet)
{
    return packet_encode("fovpt_packet_encode", false, c, lp, nullptr, in_rgba, sequence, out_packet);
}
int fovpt_packet_submit(fovpt_ctx* c, const fovpt_launch_params* lp, const uint32_t* in_rgba, uint32_t sequence, int* slot)
{
    return packet_submit("fovpt_packet_submit", false, c, lp, nullptr, in_rgba, sequence, slot);
}

void fovpt_packet_defaults(fovpt_packet_config* cfg)
{
    if (!cfg) return;
    for (uint32_t& k : cfg->codec) k = FOVPT_PACKET_BY_FILL;
    cfg->_reserved = 0;
}
int fovpt_packet_describe_coded(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_packet_config* cfg, uint32_t sequence, fovpt_packet_header* out)
{
    return packet_describe("fovpt_packet_describe_coded", true, c, lp, cfg, sequence, out);
}
int fovpt_packet_encode_coded(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_packet_config* cfg, const uint32_t* in_rgba, uint32_t sequence,
                              void* out_packet)
{
    return packet_encode("fovpt_packet_encode_coded", true, c, lp, cfg, in_rgba, sequence, out_packet);
}
int fovpt_packet_submit_coded(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_packet_config* cfg, const uint32_t* in_rgba, uint32_t sequence,
                              int* slot)
{
    return packet_submit("fovpt_packet_submit_coded", true, c, lp, cfg, in_rgba, sequence, slot);
}

int fovpt_packet_wait(fovpt_ctx* c, int slot, const void** packet, size_t* bytes)
{
    const char* who = "fovpt_packet_wait";
    if (!c) return FOVPT_E_INVALID;
    if (!packet || !bytes) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    if (slot < 0 || slot >= FOVPT_PACKET_SLOTS) return fail(c, FOVPT_E_INVALID, "%s: slot %d outside 0 .. %d", who, slot, FOVPT_PACKET_SLOTS - 1);
    fovpt_ctx::PacketSlot& S = c->pk_slot[slot];
    if (!S.submitted) return fail(c, FOVPT_E_INVALID, "%s: slot %d was never submitted", who, slot);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventSynchronize(S.ev_done));
    *packet = S.host;
    *bytes = S.bytes;
    return FOVPT_OK;
}

int fovpt_packet_decode(fovpt_ctx* c, const fovpt_packet_header* header, const void* packet, int mode, uint32_t* out_rgba)
{
    const char* who = "fovpt_packet_decode";
    if (!c) return FOVPT_E_INVALID;
    if (!header || !packet || !out_rgba) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    if (mode != FOVPT_PACKET_NEAREST && mode != FOVPT_PACKET_SMOOTH) return fail(c, FOVPT_E_INVALID, "%s: unknown mode %d", who, mode);
    if (((uintptr_t)packet & 3u) != 0u) return fail(c, FOVPT_E_INVALID, "%s: the packet is not 4-byte aligned", who);
    PacketArgs a;
    memset(&a, 0, sizeof(a));
    a.h = *header;
    if (const char* why = fovpt_packet_header_error(&a.h, a.h.bytes)) return fail(c, FOVPT_E_INVALID, "%s: %s", who, why);
    for (uint32_t p = 0; p < a.h.npass; p++) {
        // the search for a pixel's last texel takes l * factor + off as a signed sum (fovpt_pixel.h, writer_range)
        const fovpt_packet_pass& P = a.h.pass[p];
        const uint64_t far = (uint64_t)((P.gw > P.gh ? P.gw : P.gh) - 1u) * (uint64_t)P.factor;
        if (far + FOVPT_PACKET_MAX_FILL > 0x7fffffffull)
            return fail(c, FOVPT_E_INVALID, "%s: pass %u reaches pixel index %llu: beyond the device decoder (fovpt_packet_decode_host decodes it)", who, p,
                        (unsigned long long)far);
    }
    HIPCHK(c, hipSetDevice(c->device));
    fovpt_launch_packet_decode(c->shadow_stream, a, mode, (const uint32_t*)packet, out_rgba);
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

}  // extern "C"
