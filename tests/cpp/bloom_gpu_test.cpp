// fovpt_bloom through the drop-in C++ API: the box scene of post_gpu_test.cpp rendered, stepped with SampleRenderer::post(), then
// bloomPost() with Karis weights, per-level gains and a lowered threshold, and exposeBloom() behind it; once more with the defaults
// straight from the accum buffer.  Writes the two bloom colours (float4), their rgba8 and the exposed rgba8 to a file.
#include <cstdio>
#include <vector>
#include "SimplePathtracer.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "bloom_out.bin";
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
        std::vector<fovpt_float4> color(n * 2);
        std::vector<uint32_t> pixels(n * 3);
        fovpt_bloom_config bc;
        if (fovpt_bloom_defaults(&bc) != FOVPT_OK) { printf("fovpt_bloom_defaults failed\n"); return 2; }
        bc.flags = FOVPT_BLOOM_KARIS | FOVPT_BLOOM_GAINS;
        bc.levels = 5; bc.threshold = 0.5f; bc.exposure = 1.0f; bc.intensity = 0.25f;
        bc.gain_fovea = 1.0f; bc.gain_middle = 0.5f; bc.gain_periphery = 0.25f;
        fovpt_expose_config ec;
        if (fovpt_expose_defaults(&ec) != FOVPT_OK) { printf("fovpt_expose_defaults failed\n"); return 2; }
        ec.mode = FOVPT_EXPOSE_FIXED; ec.exposure = 2.0f;
        sample.render();
        sample.post();
        sample.bloomPost(bc);
        sample.downloadBloomColor(color.data());
        sample.downloadBloomPixels(pixels.data());
        sample.exposeBloom(ec);
        sample.downloadExposedPixels(pixels.data() + n);
        sample.bloom();
        sample.downloadBloomColor(color.data() + n);
        sample.downloadBloomPixels(pixels.data() + 2 * n);
        FILE* f = fopen(out, "wb");
        fwrite(color.data(), sizeof(fovpt_float4), color.size(), f);
        fwrite(pixels.data(), 4, pixels.size(), f);
        fclose(f);
        // more levels than the stage has are refused
        bool threw = false;
        bc.levels = FOVPT_BLOOM_MAX_LEVELS + 1;
        try { sample.bloom(bc); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { printf("bloom(levels 9) did not throw\n"); return 2; }
        printf("ok\n");
        delete model;
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
