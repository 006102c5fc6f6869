// fovpt_variance / fovpt_variance_filter through the drop-in C++ API: the box scene of lens_gpu_test.cpp rendered twice (two
// subframes), a moment step after each, then the raw frame filtered with the defaults and with five iterations and no demodulation.
// Writes the two rgba8 frames, the two float4 frames and the variance image to a file.
#include <cstdio>
#include <cstring>
#include <vector>
#include "SimplePathtracer.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "variance_out.bin";
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
        std::vector<uint32_t> pixels(n * 2);
        std::vector<fovpt_float4> colors(n * 2), var(n);
        // before any render the stage has no frame: an exception, like every other error of the shim
        bool threw = false;
        try { sample.variance(); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { printf("variance() before any render did not throw\n"); return 2; }
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
        FILE* f = fopen(out, "wb");
        fwrite(pixels.data(), 4, pixels.size(), f);
        fwrite(colors.data(), 16, colors.size(), f);
        fwrite(var.data(), 16, var.size(), f);
        fclose(f);
        // an iteration count out of range is an exception too
        threw = false;
        fc.iterations_middle = FOVPT_DENOISE_MAX_ITERATIONS + 1;
        try { sample.varianceFilter(fc); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { printf("varianceFilter(6 iterations) did not throw\n"); return 2; }
        printf("ok\n");
        delete model;
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
