// fovpt_focus through the drop-in C++ API: the box scene of post_gpu_test.cpp rendered and stepped with SampleRenderer::post(), then
// the post colour focused twice with the defaults' meter and a strength that blurs the slab -- once with the post step's G-buffer
// (focusPost), once tracing its own -- and the raw frame focused at a fixed distance.  Writes the three rgba8 frames, the three
// float4 frames and the two state records to a file.
#include <cstdio>
#include <cstring>
#include <vector>
#include "SimplePathtracer.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "focus_out.bin";
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
        std::vector<fovpt_float4> colors(n * 3);
        struct fovpt_focus_state states[2];
        struct fovpt_focus_state none = sample.focusState();
        if (none.steps || none.count || none.focus != 0.0f) { printf("the state before any focus is not zero\n"); return 2; }
        sample.render();
        sample.post();
        fovpt_focus_config fc;
        if (fovpt_focus_defaults(&fc) != FOVPT_OK) { printf("fovpt_focus_defaults failed\n"); return 2; }
        fc.strength = 40.0f;
        sample.focusPost(fc);
        sample.downloadFocus(colors.data(), pixels.data());
        states[0] = sample.focusState();
        fovpt_float4* post_color = nullptr;
        uint32_t* post_rgba = nullptr;
        if (fovpt_post_buffers(sample.context(), &post_color, &post_rgba) != FOVPT_OK) { printf("fovpt_post_buffers failed\n"); return 2; }
        sample.focus(fc, false, post_color);
        sample.downloadFocus(colors.data() + n, pixels.data() + n);
        states[1] = sample.focusState();
        if (memcmp(pixels.data(), pixels.data() + n, n * 4) != 0 || memcmp(colors.data(), colors.data() + n, n * 16) != 0) {
            printf("the post step's G-buffer gives another image than the call's own trace\n");
            return 2;
        }
        if (states[0].steps != 1 || states[1].steps != 2 || states[0].count == 0 || states[0].focus != states[1].focus) {
            printf("the state records are not those of two steps on one frame\n");
            return 2;
        }
        fc.mode = FOVPT_FOCUS_FIXED; fc.focus_distance = 9.0f; fc.max_radius = FOVPT_FOCUS_MAX_RADIUS;
        fc.strength = sample.focusStrength(0.4f);
        sample.focus(fc);
        sample.downloadFocus(colors.data() + 2 * n, pixels.data() + 2 * n);
        if (sample.focusState().steps != 2) { printf("a FIXED call touched the state\n"); return 2; }
        FILE* f = fopen(out, "wb");
        fwrite(pixels.data(), 4, pixels.size(), f);
        fwrite(colors.data(), 16, colors.size(), f);
        fwrite(states, sizeof(states[0]), 2, f);
        fwrite(&fc.strength, 4, 1, f);
        fclose(f);
        sample.focusReset();
        if (sample.focusState().steps != 0) { printf("focusReset left the state\n"); return 2; }
        // an out-of-range configuration is an exception, like every other error of the shim
        bool threw = false;
        fc.max_radius = FOVPT_FOCUS_MAX_RADIUS + 1;
        try { sample.focus(fc); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { printf("focus(max_radius %d) did not throw\n", FOVPT_FOCUS_MAX_RADIUS + 1); return 2; }
        printf("ok\n");
        delete model;
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
