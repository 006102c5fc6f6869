// Compile check (tests/test_packet_bc_cpu.py, g++ -fsyntax-only): the coded-packet overload of SampleRenderer::submitPacket and
// the C declarations it rests on, as an application would write them.
#include "SimplePathtracer.h"

int coded_packets(SampleRenderer& sample, uint32_t* out, int w, int h)
{
    fovpt_packet_config codec;
    fovpt_packet_defaults(&codec);                            // BC1 where a pass's fill is above 1
    const int a = sample.submitPacket(1u, codec);
    codec.codec[0] = FOVPT_PACKET_BC1; codec.codec[1] = FOVPT_PACKET_BC1; codec.codec[2] = FOVPT_PACKET_RAW;
    const int b = sample.submitPacket(2u, codec, nullptr);
    const int c = sample.submitPacket(3u);                    // raw and coded submits share the slots
    const SampleRenderer::Packet p = sample.waitPacket(a);
    fovpt_packet_header hd;
    const fovpt_launch_params* lp = reinterpret_cast<const fovpt_launch_params*>(&sample.launchParams);
    if (fovpt_packet_describe_coded(sample.context(), lp, &codec, 2u, &hd) != FOVPT_OK || hd.magic != FOVPT_PACKET_MAGIC_CODED) return -1;
    if (fovpt_packet_check(p.data, p.bytes) != FOVPT_OK) return -1;
    if (fovpt_packet_decode_host(p.data, p.bytes, FOVPT_PACKET_SMOOTH, out, w, h) != FOVPT_OK) return -1;
    return b + c;
}
