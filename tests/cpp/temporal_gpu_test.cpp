// The temporal reprojection through the drop-in C++ API: the box scene of shim_gpu_test.cpp rendered, SampleRenderer::temporal()
// and downloadTemporalPixels, then the camera moved, a second frame and a second temporal step.  Writes the first step's rgba8
// frame, the second rgba8 frame and the second step's rgba8 frame to a file.
#include <cstdio>
#include <vector>
#include "SimplePathtracer.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "temporal_out.bin";
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
        cfg.write_guides = 1;
        sample.setConfig(cfg);
        sample.launchParams.frame.c.x = fbSize.x / 2;
        sample.launchParams.frame.c.y = fbSize.y / 2;
        sample.launchParams.frame.subframe_index = 0;
        std::vector<uint32_t> pixels(n * 3);
        sample.render();
        sample.temporal();
        sample.downloadTemporalPixels(pixels.data());
        sutil::Camera moved(make_float3(3.5f, 3, 6.5f), make_float3(0, 0.5f, 0), make_float3(0, 1, 0), 45.0f, fbSize.x / float(fbSize.y));
        sample.setCamera(moved);
        sample.render();
        sample.downloadPixels(pixels.data() + n);
        sample.temporal();
        sample.downloadTemporalPixels(pixels.data() + 2 * n);
        FILE* f = fopen(out, "wb");
        fwrite(pixels.data(), 4, pixels.size(), f);
        fclose(f);
        // an out-of-range configuration is an exception, like every other error of the shim
        bool threw = false;
        fovpt_temporal_config bad;
        fovpt_temporal_defaults(&bad);
        bad.history_periphery = FOVPT_TEMPORAL_MAX_HISTORY + 1;
        try { sample.temporal(bad); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { printf("temporal(history_periphery %d) did not throw\n", FOVPT_TEMPORAL_MAX_HISTORY + 1); return 2; }
        sample.temporal_reset();
        printf("ok\n");
        delete model;
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
