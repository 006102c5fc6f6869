// api_packet.hip -- foveated frame packets, raw and coded, over the C ABI (include/fovpt.h, fovpt_packet_*): the header of the frame as rendered,
// the encoder (packet.hip) on fovpt_stream(), the slots that take a packet to pinned host memory on a copy stream of the
// context's own, and the device decoder.  The decoder for a client and the checks are packet_host.cpp.
#include <cmath>
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

// A checked submit of a packet of `bytes` bytes, of any kind: encode(out) enqueues the encoder into the slot's own device buffer
// on fovpt_stream() (FOVPT_OK or its error); an event behind it, and on the copy stream -- which waits for that event and for
// nothing else -- the copy into the slot's pinned buffer and the slot's done-event.  The host waits only for the previous copy
// out of the slot it is about to reuse, if that is still running.
template <class Encode>
int slot_submit(fovpt_ctx* c, size_t bytes, Encode encode, int* slot)
{
    HIPCHK(c, hipSetDevice(c->device));
    CHK(packet_slots(c));
    const int k = (int)(c->pk_next % FOVPT_PACKET_SLOTS);
    fovpt_ctx::PacketSlot& S = c->pk_slot[k];
    if (S.submitted) HIPCHK(c, hipEventSynchronize(S.ev_done));
    if (S.host_bytes < bytes) {                                       // (the packet's size follows the frame's size and the radii, not the gaze)
        if (S.host) (void)hipHostFree(S.host);
        S.host = nullptr; S.host_bytes = 0; S.submitted = false;
        HIPCHK(c, hipHostMalloc(&S.host, bytes, hipHostMallocDefault));
        S.host_bytes = bytes;
    }
    HIPCHK(c, S.dev.reserve(bytes));
    CHK(encode((uint32_t*)S.dev.p));
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

// The device decoders' search for a pixel's last texel takes l * factor + off as a signed sum (fovpt_pixel.h, writer_range): a
// checked header whose passes reach further is for the host decoder (`host`: its name, for the error text).
int check_decoder_reach(fovpt_ctx* c, const fovpt_packet_header& h, const char* who, const char* host)
{
    for (uint32_t p = 0; p < h.npass; p++) {
        const fovpt_packet_pass& P = h.pass[p];
        const uint64_t far = (uint64_t)((P.gw > P.gh ? P.gw : P.gh) - 1u) * (uint64_t)P.factor;
        if (far + FOVPT_PACKET_MAX_FILL > 0x7fffffffull)
            return fail(c, FOVPT_E_INVALID, "%s: pass %u reaches pixel index %llu: beyond the device decoder (%s decodes it)", who, p,
                        (unsigned long long)far, host);
    }
    return FOVPT_OK;
}

int packet_submit(const char* who, bool coded, fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_packet_config* cfg, const uint32_t* in_rgba,
                  uint32_t sequence, int* slot)
{
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !slot || (coded && !cfg)) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    PacketArgs a;
    CHK(packet_args(c, lp, cfg, sequence, who, a));
    const uint32_t* in = packet_input(lp, in_rgba);
    if (!in) return fail(c, FOVPT_E_NO_FRAME, "%s: null frame_buffer", who);
    return slot_submit(c, a.h.bytes, [&](uint32_t* out) { launch_encode(c, a, in, out); return (int)FOVPT_OK; }, slot);
}

// ---- the depth packet ("FVPD") ---------------------------------------------------------------------------------------------------
// What describe_depth, encode_depth and submit_depth (`who`) ask beyond packet_args, whose pass records these are: a config with a
// usable near, a rendered camera that has an inverse, and a G-buffer of the frame's size (or, with none, the scene to trace one).
// Fills the kernels' arguments; nothing is allocated, enqueued or changed.
int packet_depth_args(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_packet_depth_config* cfg, const fovpt_gbuffer_ptrs* gbuffer,
                      bool need_gbuffer, uint32_t sequence, const char* who, PacketDepthArgs& a)
{
    if (cfg->_reserved[0] | cfg->_reserved[1] | cfg->_reserved[2]) return fail(c, FOVPT_E_INVALID, "%s: non-zero reserved word in the depth packet config", who);
    if (!(std::isfinite(cfg->near) && cfg->near > 0.0f)) return fail(c, FOVPT_E_INVALID, "%s: near %g is not finite and above 0", who, (double)cfg->near);
    PacketArgs raw;
    CHK(packet_args(c, lp, nullptr, sequence, who, raw));
    if (need_gbuffer && !gbuffer && (!c->has_scene || lp->traversable != c->scene_id)) return fail(c, FOVPT_E_NO_SCENE, "%s without a scene", who);
    if (gbuffer && (gbuffer->width != c->rendered.w || gbuffer->height != c->rendered.h || !gbuffer->prim || !gbuffer->position))
        return fail(c, FOVPT_E_INVALID, "%s: the G-buffer is not of the frame's size %d x %d, or has a null prim or position", who, c->rendered.w, c->rendered.h);
    const FrameDev& fd = c->rendered.frame;
    memset(&a, 0, sizeof(a));
    fovpt_packet_header& h = a.h.base;
    h = raw.h;
    h.magic = FOVPT_PACKET_MAGIC_DEPTH;
    uint64_t at = FOVPT_PACKET_DEPTH_HEADER_BYTES;
    for (uint32_t p = 0; p < h.npass; p++) {
        h.pass[p].texels = (uint32_t)at;
        at += fovpt_packet_depth_pass_bytes(h.pass[p].gw, h.pass[p].gh);
    }
    h.bytes = (uint32_t)at;                                           // (<= 192 + 2^27 + 12)
    memcpy(a.first, raw.first, sizeof(a.first));
    memcpy(&a.h.camera.eye.x, fd.eye, 12); memcpy(&a.h.camera.U.x, fd.U, 12);
    memcpy(&a.h.camera.V.x, fd.V, 12); memcpy(&a.h.camera.W.x, fd.W, 12);
    a.h.near = cfg->near;
    float inv[9];
    if (!camera_inverse(fd.U, fd.V, fd.W, inv)) return fail(c, FOVPT_E_INVALID, "%s: the rendered camera is singular", who);
    memcpy(a.m2, inv + 6, sizeof(a.m2));
    if (const char* why = fovpt_packet_depth_header_error(&a.h, at)) return fail(c, FOVPT_E_INVALID, "%s: the frame does not fit a depth packet: %s", who, why);
    return FOVPT_OK;
}

// the trace of the rendered frame's G-buffer where the caller gave none (the same stream, into fovpt_gbuffer's buffers), then the encoder
int packet_depth_enqueue(fovpt_ctx* c, const fovpt_launch_params* lp, const PacketDepthArgs& a, const fovpt_gbuffer_ptrs* gbuffer, uint32_t* out,
                         const char* who)
{
    GBufferDev g = gbuffer_dev(c, gbuffer);
    if (!gbuffer) CHK(enqueue_gbuffer(c, lp, c->rendered.frame, g, who));
    fovpt_launch_packet_depth_encode(c->shadow_stream, c->rendered.frame, a, g.prim, g.pos, out);
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
    CHK(check_decoder_reach(c, a.h, who, "fovpt_packet_decode_host"));
    HIPCHK(c, hipSetDevice(c->device));
    fovpt_launch_packet_decode(c->shadow_stream, a, mode, (const uint32_t*)packet, out_rgba);
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

// ---- the depth packet ("FVPD": packet.hip, k_packet_depth_*; its definition: tests/packet_depth_ref.py) --------------------------
// (fovpt_packet_depth_defaults, which needs no context, is beside the checks in packet_host.cpp)
int fovpt_packet_describe_depth(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_packet_depth_config* cfg, uint32_t sequence,
                                fovpt_packet_depth_header* out)
{
    const char* who = "fovpt_packet_describe_depth";
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !cfg || !out) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    PacketDepthArgs a;
    CHK(packet_depth_args(c, lp, cfg, nullptr, false, sequence, who, a));
    *out = a.h;
    return FOVPT_OK;
}

// Enqueued on fovpt_stream() like fovpt_packet_encode, and ordered like it.
int fovpt_packet_encode_depth(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_packet_depth_config* cfg, const fovpt_gbuffer_ptrs* gbuffer,
                              uint32_t sequence, void* out_packet)
{
    const char* who = "fovpt_packet_encode_depth";
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !cfg || !out_packet) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    if (((uintptr_t)out_packet & 3u) != 0u) return fail(c, FOVPT_E_INVALID, "%s: the packet buffer is not 4-byte aligned", who);
    PacketDepthArgs a;
    CHK(packet_depth_args(c, lp, cfg, gbuffer, true, sequence, who, a));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(packet_depth_enqueue(c, lp, a, gbuffer, (uint32_t*)out_packet, who));
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

int fovpt_packet_submit_depth(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_packet_depth_config* cfg, const fovpt_gbuffer_ptrs* gbuffer,
                              uint32_t sequence, int* slot)
{
    const char* who = "fovpt_packet_submit_depth";
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !cfg || !slot) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    PacketDepthArgs a;
    CHK(packet_depth_args(c, lp, cfg, gbuffer, true, sequence, who, a));
    return slot_submit(c, a.h.base.bytes, [&](uint32_t* out) { return packet_depth_enqueue(c, lp, a, gbuffer, out, who); }, slot);
}

int fovpt_packet_decode_depth(fovpt_ctx* c, const fovpt_packet_depth_header* header, const void* packet, float* out_depth)
{
    const char* who = "fovpt_packet_decode_depth";
    if (!c) return FOVPT_E_INVALID;
    if (!header || !packet || !out_depth) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    if (((uintptr_t)packet & 3u) != 0u) return fail(c, FOVPT_E_INVALID, "%s: the packet is not 4-byte aligned", who);
    PacketDepthArgs a;
    memset(&a, 0, sizeof(a));
    a.h = *header;
    if (const char* why = fovpt_packet_depth_header_error(&a.h, a.h.base.bytes)) return fail(c, FOVPT_E_INVALID, "%s: %s", who, why);
    CHK(check_decoder_reach(c, a.h.base, who, "fovpt_packet_decode_depth_host"));
    HIPCHK(c, hipSetDevice(c->device));
    fovpt_launch_packet_depth_decode(c->shadow_stream, a, (const uint32_t*)packet, out_depth);
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

}  // extern "C"
