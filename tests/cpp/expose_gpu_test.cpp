// fovpt_expose through the drop-in C++ API: the box scene of post_gpu_test.cpp rendered, stepped with SampleRenderer::post() and
// exposed with exposePost() twice (defaults but adapt rates 0.5, so the second step is a blend), then once more with a fixed
// exposure and the ACES curve straight from the accum buffer.  Writes the three rgba8 frames and the two states to a file.
#include <cstdio>
#include <vector>
#include "SimplePathtracer.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "expose_out.bin";
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
        struct fovpt_expose_state st[2];
        fovpt_expose_config ec;
        if (fovpt_expose_defaults(&ec) != FOVPT_OK) { printf("fovpt_expose_defaults failed\n"); return 2; }
        ec.adapt_brighter = ec.adapt_darker = 0.5f;
        for (int k = 0; k < 2; k++) {
            sample.launchParams.frame.c.x = fbSize.x / 2 + 40 * k;          // the second frame looks at the sky
            sample.launchParams.frame.c.y = fbSize.y / 2 - 30 * k;
            sample.render();
            sample.post();
            sample.exposePost(ec);
            sample.downloadExposedPixels(pixels.data() + k * n);
            st[k] = sample.exposeState();
        }
        ec.mode = FOVPT_EXPOSE_FIXED; ec.tone = FOVPT_TONE_ACES; ec.exposure = 0.75f;
        sample.expose(ec);
        sample.downloadExposedPixels(pixels.data() + 2 * n);
        struct fovpt_expose_state after = sample.exposeState();
        if (after.steps != 2 || after.ev != st[1].ev) { printf("a FIXED call moved the state\n"); return 2; }
        FILE* f = fopen(out, "wb");
        fwrite(pixels.data(), 4, pixels.size(), f);
        fwrite(st, sizeof(st[0]), 2, f);
        fclose(f);
        // an unknown tone map is refused
        bool threw = false;
        ec.tone = 2;
        try { sample.expose(ec); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { printf("expose(tone 2) did not throw\n"); return 2; }
        sample.exposeReset();
        if (sample.exposeState().steps != 0) { printf("exposeReset left steps\n"); return 2; }
        printf("ok\n");
        delete model;
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
