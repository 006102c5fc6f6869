// The reconstruction through the drop-in C++ API: the box scene of box_scene.h rendered with the denoiser guides, then
// SampleRenderer::reconstruct() and downloadReconstructedPixels.  Writes the rgba8 frame and the reconstructed rgba8 frame to
// a file.
#include <cstdio>
#include <vector>
#include "box_scene.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "reconstruct_out.bin";
    return run_main([&]() -> int {
        BoxScene scene;

        SampleRenderer sample(scene.model);
        scene.setup(sample, true);
        sample.render();
        sample.reconstruct();
        std::vector<uint32_t> pixels((size_t)scene.fbSize.x * scene.fbSize.y * 2);
        sample.downloadPixels(pixels.data());
        sample.downloadReconstructedPixels(pixels.data() + (size_t)scene.fbSize.x * scene.fbSize.y);
        OutFile f(out);
        f.write(pixels.data(), 4, pixels.size());
        f.close();
        // an out-of-range configuration is an exception, like every other error of the shim
        fovpt_reconstruct_config bad;
        fovpt_reconstruct_defaults(&bad);
        bad.support = 3.0f;
        if (!must_throw([&] { sample.reconstruct(bad); }, "reconstruct(support 3) did not throw")) return 2;
        printf("ok\n");
        return 0;
    });
}
