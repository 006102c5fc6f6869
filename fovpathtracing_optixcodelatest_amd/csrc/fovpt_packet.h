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
void fovpt_launch_packet_decode(hipStream_t st, const PacketArgs& a, int mode, const uint32_t* packet, uint32_t* out);
#endif
