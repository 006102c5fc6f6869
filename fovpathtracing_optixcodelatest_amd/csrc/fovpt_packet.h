// fovpt_packet.h -- the foveated frame packet (include/fovpt.h, fovpt_packet_*): what packet_host.cpp
// (host-only C++, also in libfovpt_loader.so), packet.hip (the kernels) and api_packet.hip (the context's entry points) share.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/fovpt.h"

#define FOVPT_PACKET_HEADER_BYTES 128u
#define FOVPT_PACKET_MAX_DIM 16384
#define FOVPT_PACKET_MAX_TEXELS (1ull << 26)
#define FOVPT_PACKET_MAX_FILL 8u

// The checks of fovpt_packet_check on a header alone, `avail` the bytes the caller holds (packet_host.cpp).  Null: the header is
// valid; otherwise what is wrong with it.
const char* fovpt_packet_header_error(const fovpt_packet_header* h, uint64_t avail);
// The same for a depth packet's header ("FVPD", 192 bytes: the pass records, the rendered camera, near)
const char* fovpt_packet_depth_header_error(const fovpt_packet_depth_header* h, uint64_t avail);
// the bytes of a depth pass's array: gw * gh uint16 codes, rounded up to a multiple of 4, in 64 bits
inline uint64_t fovpt_packet_depth_pass_bytes(uint32_t gw, uint32_t gh) { return (2ull * (uint64_t)gw * (uint64_t)gh + 3ull) & ~3ull; }
// the bytes of a pass's array under a codec (FOVPT_PACKET_RAW / _BC1), in 64 bits
inline uint64_t fovpt_packet_pass_bytes(uint32_t gw, uint32_t gh, uint32_t codec)
{
    return codec == FOVPT_PACKET_BC1 ? 8ull * (((uint64_t)gw + 3u) >> 2) * (((uint64_t)gh + 3u) >> 2) : 4ull * (uint64_t)gw * (uint64_t)gh;
}

#ifdef __HIP__
#include "fovpt_device.h"

// What both kernels take by value: the header as it is written / was checked, and the first texel of each pass in the
// concatenated texel arrays (first[npass] = their total; the encoder's arrays follow the header back to back, the decoder goes
// by each pass's own byte offset).
struct PacketArgs {
    fovpt_packet_header h;
    uint32_t first[FOVPT_MAX_PASSES + 1];
};
// fd: the frame as rendered (fovpt_ctx::dn_frame), whose passes a.h describes.  in: the rgba8 image; out: the packet.
void fovpt_launch_packet_encode(hipStream_t st, const FrameDev& fd, const PacketArgs& a, const uint32_t* in, uint32_t* out);
// A coded packet ("FVPC", a.h.pass[p]._reserved the codec): first[p] is the first thread of pass p, a multiple of 16 -- a raw
// pass takes one thread per texel, a BC1 pass 16 per block --, first[npass] their total; the arrays go by their byte offsets.
void fovpt_launch_packet_encode_coded(hipStream_t st, const FrameDev& fd, const PacketArgs& a, const uint32_t* in, uint32_t* out);
// (either magic: a coded header runs the CODED instantiation)
void fovpt_launch_packet_decode(hipStream_t st, const PacketArgs& a, int mode, const uint32_t* packet, uint32_t* out);
// The depth packet's kernels take its header, first[] as the raw encoder's (texels before each pass, their total) and the third
// row of the rendered camera's inverse (the encoder alone reads the last two).
struct PacketDepthArgs {
    fovpt_packet_depth_header h;
    uint32_t first[FOVPT_MAX_PASSES + 1];
    float m2[3];
};
// fd: the frame as rendered; prim, pos: its G-buffer; out: the packet, written whole (header, codes, padding)
void fovpt_launch_packet_depth_encode(hipStream_t st, const FrameDev& fd, const PacketDepthArgs& a, const uint32_t* prim, const float4* pos,
                                      uint32_t* out);
// out: h.base.width x height floats; a pixel no texel reaches is not written
void fovpt_launch_packet_depth_decode(hipStream_t st, const PacketDepthArgs& a, const uint32_t* packet, float* out);
#endif
