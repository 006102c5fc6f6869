// Foveated frame packets through the drop-in C++ API: the box scene of post_gpu_test.cpp rendered at three gazes, each frame
// submitted as a packet the moment it is issued and the next one rendered at once; then every slot is waited for, checked, decoded
// on the host (fovpt_packet_decode_host, both modes) and compared with what downloadPixels gave for that frame.  Writes the
// packets' sizes, the three downloaded frames and the three NEAREST decodes to a file.
#include <cstdio>
#include <cstring>
#include <vector>
#include "SimplePathtracer.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "packet_out.bin";
    try {
        Model* model = new Model;
        Material grey; grey.color = make_float3(0.7f, 0.7f, 0.7f); grey.emission = make_float3(0.0f);
        Material red; red.color = make_float3(0.8f, 0.1f, 0.1f); red.emission = make_float3(0.0f);
        addBox(model, grey, make_float3(0, -1.0f, 0), make_float3(6, 0.5f, 6));
        addBox(model, red, make_float3(0, 0.5f, 0), make_float3(1, 1, 1));
        const int2 fbSize = make_int2(160, 96);
        const size_t n = (size_t)fbSize.x * fbSize.y;
        std::vector<float4> sky(n, make_float4(2.5f, 2.5f, 2.5f, 1.0f));
        ProbeData probe;
        probe.width = fbSize.x; probe.height = fbSize.y; probe.data = sky.data();
        probe.BuildCDF();
        sutil::Camera camera(make_float3(4, 3, 6), make_float3(0, 0.5f, 0), make_float3(0, 1, 0), 45.0f, fbSize.x / float(fbSize.y));

        SampleRenderer sample(model);
        sample.resize(fbSize);
        sample.setCamera(camera);
        sample.setProbe(probe);
        fovpt_config cfg = sample.config();
        cfg.r_inner = 12; cfg.r_outer = 36; cfg.spp_periphery = 1; cfg.spp_middle = 2; cfg.spp_fovea = 8;
        sample.setConfig(cfg);
        sample.launchParams.frame.subframe_index = 0;
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
            if (fovpt_packet_decode_host(p.data, p.bytes, FOVPT_PACKET_NEAREST, decoded.data() + k * n, fbSize.x, fbSize.y) != FOVPT_OK) { printf("decode %d failed\n", k); return 2; }
            if (fovpt_packet_decode_host(p.data, p.bytes, FOVPT_PACKET_SMOOTH, smooth.data(), fbSize.x, fbSize.y) != FOVPT_OK) { printf("smooth decode %d failed\n", k); return 2; }
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
        bool threw = false;
        try { sample.waitPacket(3); } catch (const std::runtime_error&) { threw = true; }      // never submitted
        if (!threw) { printf("waitPacket(3) did not throw\n"); return 2; }
        FILE* f = fopen(out, "wb");
        fwrite(sizes, 4, 3, f);
        fwrite(frames.data(), 4, frames.size(), f);
        fwrite(decoded.data(), 4, decoded.size(), f);
        fclose(f);
        printf("ok\n");
        delete model;
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
