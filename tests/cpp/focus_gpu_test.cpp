// fovpt_focus through the drop-in C++ API: the box scene of box_scene.h rendered and stepped with SampleRenderer::post(), then
// the post colour focused twice with the defaults' meter and a strength that blurs the slab -- once with the post step's G-buffer
// (focusPost), once tracing its own -- and the raw frame focused at a fixed distance.  Writes the three rgba8 frames, the three
// float4 frames and the two state records to a file.
#include <cstdio>
#include <cstring>
#include <vector>
#include "box_scene.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "focus_out.bin";
    return run_main([&]() -> int {
        BoxScene scene;
        const size_t n = scene.n;

        SampleRenderer sample(scene.model);
        scene.setup(sample, true);
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
        OutFile f(out);
        f.write(pixels.data(), 4, pixels.size());
        f.write(colors.data(), 16, colors.size());
        f.write(states, sizeof(states[0]), 2);
        f.write(&fc.strength, 4, 1);
        f.close();
        sample.focusReset();
        if (sample.focusState().steps != 0) { printf("focusReset left the state\n"); return 2; }
        // an out-of-range configuration is an exception, like every other error of the shim
        fc.max_radius = FOVPT_FOCUS_MAX_RADIUS + 1;
        if (!must_throw([&] { sample.focus(fc); }, text("focus(max_radius %d) did not throw", FOVPT_FOCUS_MAX_RADIUS + 1))) return 2;
        printf("ok\n");
        return 0;
    });
}
