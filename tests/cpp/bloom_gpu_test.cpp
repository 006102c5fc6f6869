// fovpt_bloom through the drop-in C++ API: the box scene of box_scene.h rendered, stepped with SampleRenderer::post(), then
// bloomPost() with Karis weights, per-level gains and a lowered threshold, and exposeBloom() behind it; once more with the defaults
// straight from the accum buffer.  Writes the two bloom colours (float4), their rgba8 and the exposed rgba8 to a file.
#include <cstdio>
#include <vector>
#include "box_scene.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "bloom_out.bin";
    return run_main([&]() -> int {
        BoxScene scene;
        const size_t n = scene.n;

        SampleRenderer sample(scene.model);
        scene.setup(sample, true);
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
        OutFile f(out);
        f.write(color.data(), sizeof(fovpt_float4), color.size());
        f.write(pixels.data(), 4, pixels.size());
        f.close();
        // more levels than the stage has are refused
        bc.levels = FOVPT_BLOOM_MAX_LEVELS + 1;
        if (!must_throw([&] { sample.bloom(bc); }, "bloom(levels 9) did not throw")) return 2;
        printf("ok\n");
        return 0;
    });
}
