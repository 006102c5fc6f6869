// fovpt_expose through the drop-in C++ API: the box scene of box_scene.h rendered, stepped with SampleRenderer::post() and
// exposed with exposePost() twice (defaults but adapt rates 0.5, so the second step is a blend), then once more with a fixed
// exposure and the ACES curve straight from the accum buffer.  Writes the three rgba8 frames and the two states to a file.
#include <cstdio>
#include <vector>
#include "box_scene.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "expose_out.bin";
    return run_main([&]() -> int {
        BoxScene scene;
        const size_t n = scene.n;

        SampleRenderer sample(scene.model);
        scene.setup(sample, true);
        std::vector<uint32_t> pixels(n * 3);
        struct fovpt_expose_state st[2];
        fovpt_expose_config ec;
        if (fovpt_expose_defaults(&ec) != FOVPT_OK) { printf("fovpt_expose_defaults failed\n"); return 2; }
        ec.adapt_brighter = ec.adapt_darker = 0.5f;
        for (int k = 0; k < 2; k++) {
            sample.launchParams.frame.c.x = scene.fbSize.x / 2 + 40 * k;          // the second frame looks at the sky
            sample.launchParams.frame.c.y = scene.fbSize.y / 2 - 30 * k;
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
        OutFile f(out);
        f.write(pixels.data(), 4, pixels.size());
        f.write(st, sizeof(st[0]), 2);
        f.close();
        // an unknown tone map is refused
        ec.tone = 2;
        if (!must_throw([&] { sample.expose(ec); }, "expose(tone 2) did not throw")) return 2;
        sample.exposeReset();
        if (sample.exposeState().steps != 0) { printf("exposeReset left steps\n"); return 2; }
        printf("ok\n");
        return 0;
    });
}
