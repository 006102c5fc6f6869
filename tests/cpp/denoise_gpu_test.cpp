// The denoiser through the drop-in C++ API: the box scene of box_scene.h rendered with the denoiser guides, then
// SampleRenderer::denoise() and downloadDenoisedPixels (what the reference family's OptiXDenoiser::exec +
// computeFinalPixelColors produce for display).  Writes the rgba8 frame and the denoised rgba8 frame to a file.
#include <cstdio>
#include <vector>
#include "box_scene.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "denoise_out.bin";
    return run_main([&]() -> int {
        BoxScene scene;

        SampleRenderer sample(scene.model);
        scene.setup(sample, true);
        sample.render();
        sample.denoise();
        std::vector<uint32_t> pixels((size_t)scene.fbSize.x * scene.fbSize.y * 2);
        sample.downloadPixels(pixels.data());
        sample.downloadDenoisedPixels(pixels.data() + (size_t)scene.fbSize.x * scene.fbSize.y);
        OutFile f(out);
        f.write(pixels.data(), 4, pixels.size());
        f.close();
        // an out-of-range configuration is an exception, like every other error of the shim
        fovpt_denoise_config bad;
        fovpt_denoise_defaults(&bad);
        bad.iterations_periphery = 6;
        if (!must_throw([&] { sample.denoise(bad); }, "denoise(iterations 6) did not throw")) return 2;
        printf("ok\n");
        return 0;
    });
}
