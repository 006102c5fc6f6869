// fovpt_lens through the drop-in C++ API: the box scene of box_scene.h rendered, then the raw frame pre-distorted twice -- with
// the defaults fitted to the frame (lens()), and with Catmull-Rom taps, the resolve's encoding and a re-aim at a turned camera.
// Writes the two rgba8 frames, the two float4 frames and the fitted configuration to a file.
#include <cstdio>
#include <cstring>
#include <vector>
#include "box_scene.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "lens_out.bin";
    return run_main([&]() -> int {
        BoxScene scene;
        const size_t n = scene.n;

        SampleRenderer sample(scene.model);
        scene.setup(sample);
        std::vector<uint32_t> pixels(n * 2);
        std::vector<fovpt_float4> colors(n * 2);
        // before any render the stage has no frame: an exception, like every other error of the shim
        if (!must_throw([&] { sample.lens(); }, "lens() before any render did not throw")) return 2;
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
        sutil::Camera to(make_float3(4, 3, 6), make_float3(0.3f, 0.5f, -0.2f), make_float3(0, 1, 0), 45.0f, scene.fbSize.x / float(scene.fbSize.y));
        sample.lens(lc, &to);
        sample.downloadLens(colors.data() + n, pixels.data() + n);
        if (memcmp(pixels.data(), pixels.data() + n, n * 4) == 0) { printf("the two calls gave the same image\n"); return 2; }
        fovpt_float4* own_color = nullptr;
        uint32_t* own_rgba = nullptr;
        sample.lensBuffers(&own_color, &own_rgba);
        if (!own_color || !own_rgba) { printf("lensBuffers returned a null buffer\n"); return 2; }
        OutFile f(out);
        f.write(pixels.data(), 4, pixels.size());
        f.write(colors.data(), 16, colors.size());
        f.write(&fitted, sizeof(fitted), 1);
        f.close();
        // an unknown filter is an exception too
        lc.filter = 3;
        if (!must_throw([&] { sample.lens(lc); }, "lens(filter 3) did not throw")) return 2;
        printf("ok\n");
        return 0;
    });
}
