// fovpt_lens through the drop-in C++ API: the box scene of focus_gpu_test.cpp rendered, then the raw frame pre-distorted twice -- with
// the defaults fitted to the frame (lens()), and with Catmull-Rom taps, the resolve's encoding and a re-aim at a turned camera.
// Writes the two rgba8 frames, the two float4 frames and the fitted configuration to a file.
#include <cstdio>
#include <cstring>
#include <vector>
#include "SimplePathtracer.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "lens_out.bin";
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
        sample.launchParams.frame.c.x = fbSize.x / 2;
        sample.launchParams.frame.c.y = fbSize.y / 2;
        sample.launchParams.frame.subframe_index = 0;
        std::vector<uint32_t> pixels(n * 2);
        std::vector<fovpt_float4> colors(n * 2);
        // before any render the stage has no frame: an exception, like every other error of the shim
        bool threw = false;
        try { sample.lens(); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { printf("lens() before any render did not throw\n"); return 2; }
        sample.render();
        sample.lens();
        sample.downloadLens(colors.data(), pixels.data());
        const fovpt_lens_config fitted = sample.lensForFrame(SampleRenderer::lensDefaults());
        if (fitted.scale[1] != 96.0f / 160.0f || !(fitted.src_scale[0] < 1.0f) || fitted.filter != FOVPT_LENS_BILINEAR) {
            printf("lensForFrame(lensDefaults()) is not the documented fit\n");
            return 2;
        }
        fovpt_lens_config lc = fitted;
        lc.filter = FOVPT_LENS_BICUBIC; lc.encode = FOVPT_LENS_ENCODE_RESOLVE;
        sutil::Camera to(make_float3(4, 3, 6), make_float3(0.3f, 0.5f, -0.2f), make_float3(0, 1, 0), 45.0f, fbSize.x / float(fbSize.y));
        sample.lens(lc, &to);
        sample.downloadLens(colors.data() + n, pixels.data() + n);
        if (memcmp(pixels.data(), pixels.data() + n, n * 4) == 0) { printf("the two calls gave the same image\n"); return 2; }
        fovpt_float4* own_color = nullptr;
        uint32_t* own_rgba = nullptr;
        sample.lensBuffers(&own_color, &own_rgba);
        if (!own_color || !own_rgba) { printf("lensBuffers returned a null buffer\n"); return 2; }
        FILE* f = fopen(out, "wb");
        fwrite(pixels.data(), 4, pixels.size(), f);
        fwrite(colors.data(), 16, colors.size(), f);
        fwrite(&fitted, sizeof(fitted), 1, f);
        fclose(f);
        // an unknown filter is an exception too
        threw = false;
        lc.filter = 3;
        try { sample.lens(lc); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { printf("lens(filter 3) did not throw\n"); return 2; }
        printf("ok\n");
        delete model;
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
