// Foveated frame packets through the drop-in C++ API: the box scene of box_scene.h rendered at three gazes, each frame
// submitted as a packet the moment it is issued and the next one rendered at once; then every slot is waited for, checked, decoded
// on the host (fovpt_packet_decode_host, both modes) and compared with what downloadPixels gave for that frame.  Writes the
// packets' sizes, the three downloaded frames and the three NEAREST decodes to a file.
#include <cstdio>
#include <cstring>
#include <vector>
#include "box_scene.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "packet_out.bin";
    return run_main([&]() -> int {
        BoxScene scene;
        const size_t n = scene.n;

        SampleRenderer sample(scene.model);
        scene.setup(sample);
        const int gaze[3][2] = {{80, 48}, {150, 10}, {3, 90}};
        // the frames one by one, downloaded: what the packets must reproduce
        std::vector<uint32_t> frames(3 * n), decoded(3 * n, 0u), smooth(n);
        for (int k = 0; k < 3; k++) {
            sample.launchParams.frame.c.x = gaze[k][0]; sample.launchParams.frame.c.y = gaze[k][1];
            sample.launchParams.frame.subframe_index = k;
            sample.render();
            sample.downloadPixels(frames.data() + k * n);
        }
        // the same frames again, each submitted as a packet and none waited for until all are issued
        int slot[3];
        for (int k = 0; k < 3; k++) {
            sample.launchParams.frame.c.x = gaze[k][0]; sample.launchParams.frame.c.y = gaze[k][1];
            sample.launchParams.frame.subframe_index = k;
            const fovpt_launch_params* lp = reinterpret_cast<const fovpt_launch_params*>(&sample.launchParams);
            if (fovpt_render(sample.context(), const_cast<fovpt_launch_params*>(lp)) != FOVPT_OK) { printf("fovpt_render failed\n"); return 2; }
            slot[k] = sample.submitPacket(100u + k);
        }
        uint32_t sizes[3];
        for (int k = 0; k < 3; k++) {
            if (slot[k] != k) { printf("submit %d used slot %d\n", k, slot[k]); return 2; }
            const SampleRenderer::Packet p = sample.waitPacket(slot[k]);
            sizes[k] = (uint32_t)p.bytes;
            fovpt_packet_header h;
            memcpy(&h, p.data, sizeof(h));
            if (fovpt_packet_check(p.data, p.bytes) != FOVPT_OK || h.sequence != 100u + k || h.bytes != p.bytes || h.npass != 3) { printf("packet %d is not valid\n", k); return 2; }
            if (fovpt_packet_decode_host(p.data, p.bytes, FOVPT_PACKET_NEAREST, decoded.data() + k * n, scene.fbSize.x, scene.fbSize.y) != FOVPT_OK) { printf("decode %d failed\n", k); return 2; }
            if (fovpt_packet_decode_host(p.data, p.bytes, FOVPT_PACKET_SMOOTH, smooth.data(), scene.fbSize.x, scene.fbSize.y) != FOVPT_OK) { printf("smooth decode %d failed\n", k); return 2; }
            // every pixel a pass of frame k wrote is that frame's pixel (alpha 0xff); the others -- a few between the rings are
            // nobody's -- keep the 0 the output held
            size_t written = 0;
            for (size_t i = 0; i < n; i++) {
                const uint32_t d = decoded[k * n + i];
                if (d == 0u) continue;
                written++;
                if (d != frames[k * n + i]) { printf("frame %d pixel %zu: %08x decoded, %08x downloaded\n", k, i, d, frames[k * n + i]); return 2; }
            }
            if (written * 100 < n * 99) { printf("frame %d: only %zu pixels decoded\n", k, written); return 2; }
        }
        if (!must_throw([&] { sample.waitPacket(3); }, "waitPacket(3) did not throw")) return 2;      // never submitted
        OutFile f(out);
        f.write(sizes, 4, 3);
        f.write(frames.data(), 4, frames.size());
        f.write(decoded.data(), 4, decoded.size());
        f.close();
        printf("ok\n");
        return 0;
    });
}
