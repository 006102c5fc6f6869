// fovpt_quality through the drop-in C++ API: the box scene of post_gpu_test.cpp rendered foveated, its frame buffer measured against
// the lens stage's rgba8 image of the same frame (another image of the frame's size that lives on the device) with
// SampleRenderer::measureQuality(), then the other way round with a configuration of the caller's, then the frame buffer against
// itself through qualityAsync() / readQuality().  Writes the three records to a file.
#include <cstdio>
#include <cstring>
#include <vector>
#include "SimplePathtracer.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "quality_out.bin";
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
        sample.launchParams.frame.c.x = fbSize.x / 2 + 30;
        sample.launchParams.frame.c.y = fbSize.y / 2 - 10;
        sample.launchParams.frame.subframe_index = 0;
        sample.render();
        sample.lens();
        fovpt_float4* lens_color = nullptr;
        uint32_t* lens_rgba = nullptr;
        sample.lensBuffers(&lens_color, &lens_rgba);
        const uint32_t* frame = (const uint32_t*)sample.launchParams.frame.frame_buffer;

        fovpt_quality_sums s[3];
        s[0] = sample.measureQuality(lens_rgba);                                   // the frame buffer against the lens image, the defaults
        fovpt_quality_config qc = SampleRenderer::qualityDefaults();
        if (qc.flags != (FOVPT_QUALITY_SSIM | FOVPT_QUALITY_PROFILE) || qc.ring_width != 16) { printf("unexpected defaults\n"); return 2; }
        qc.flags = FOVPT_QUALITY_PROFILE; qc.ring_width = 5;
        s[1] = sample.measureQuality(frame, lens_rgba, &qc);
        sample.qualityAsync(frame, frame);
        s[2] = sample.readQuality();
        if (s[0].width != 160u || s[0].height != 96u || s[1].ring_width != 5u || s[1].flags != 2u) { printf("the header fields do not echo the call\n"); return 2; }
        if (fovpt_quality_mse(&s[2], -1) != 0.0 || !(fovpt_quality_mse(&s[0], -1) > 0.0) || fovpt_quality_ssim(&s[2], -1) != 1.0) { printf("unexpected scores\n"); return 2; }
        // unknown flag bits are refused, and the renderer's record stays
        bool threw = false;
        qc.flags = 4;
        try { sample.measureQuality(frame, lens_rgba, &qc); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { printf("measureQuality(flags 4) did not throw\n"); return 2; }
        const fovpt_quality_sums again = sample.readQuality();
        if (memcmp(&again, &s[2], sizeof(again)) != 0) { printf("a refused call changed the record\n"); return 2; }
        FILE* f = fopen(out, "wb");
        fwrite(s, sizeof(s[0]), 3, f);
        fclose(f);
        printf("ok\n");
        delete model;
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
