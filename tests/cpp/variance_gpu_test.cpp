// fovpt_variance / fovpt_variance_filter through the drop-in C++ API: the box scene of box_scene.h rendered twice (two
// subframes), a moment step after each, then the raw frame filtered with the defaults and with five iterations and no demodulation.
// Writes the two rgba8 frames, the two float4 frames and the variance image to a file.
#include <cstdio>
#include <cstring>
#include <vector>
#include "box_scene.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "variance_out.bin";
    return run_main([&]() -> int {
        BoxScene scene;
        const size_t n = scene.n;

        SampleRenderer sample(scene.model);
        scene.setup(sample);
        std::vector<uint32_t> pixels(n * 2);
        std::vector<fovpt_float4> colors(n * 2), var(n);
        // before any render the stage has no frame: an exception, like every other error of the shim
        if (!must_throw([&] { sample.variance(); }, "variance() before any render did not throw")) return 2;
        for (int k = 0; k < 2; k++) {
            sample.launchParams.frame.subframe_index = k;
            sample.render();
            sample.variance();
        }
        sample.varianceFilter();
        sample.downloadVarianceFiltered(pixels.data(), colors.data());
        fovpt_variance_filter_config fc = SampleRenderer::varianceFilterDefaults();
        if (fc.iterations_periphery != 4 || fc.demodulate != 1 || SampleRenderer::varianceDefaults().history_cap != 16) {
            printf("the defaults are not the documented ones\n");
            return 2;
        }
        fc.iterations_fovea = 1; fc.iterations_middle = 3; fc.iterations_periphery = 5; fc.demodulate = 0;
        sample.varianceFilter(fc);
        sample.downloadVarianceFiltered(pixels.data() + n, colors.data() + n);
        if (memcmp(pixels.data(), pixels.data() + n, n * 4) == 0) { printf("the two calls gave the same image\n"); return 2; }
        fovpt_float4* own_var = nullptr;
        const fovpt_float4* moments = nullptr;
        sample.varianceBuffers(&own_var, &moments);
        if (!own_var || !moments) { printf("varianceBuffers returned a null buffer\n"); return 2; }
        sample.downloadVariance(var.data());
        OutFile f(out);
        f.write(pixels.data(), 4, pixels.size());
        f.write(colors.data(), 16, colors.size());
        f.write(var.data(), 16, var.size());
        f.close();
        // an iteration count out of range is an exception too
        fc.iterations_middle = FOVPT_DENOISE_MAX_ITERATIONS + 1;
        if (!must_throw([&] { sample.varianceFilter(fc); }, "varianceFilter(6 iterations) did not throw")) return 2;
        printf("ok\n");
        return 0;
    });
}
