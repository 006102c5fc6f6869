// The temporal reprojection through the drop-in C++ API: the box scene of box_scene.h rendered, SampleRenderer::temporal()
// and downloadTemporalPixels, then the camera moved, a second frame and a second temporal step.  Writes the first step's rgba8
// frame, the second rgba8 frame and the second step's rgba8 frame to a file.
#include <cstdio>
#include <vector>
#include "box_scene.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "temporal_out.bin";
    return run_main([&]() -> int {
        BoxScene scene;
        const size_t n = scene.n;

        SampleRenderer sample(scene.model);
        scene.setup(sample, true);
        std::vector<uint32_t> pixels(n * 3);
        sample.render();
        sample.temporal();
        sample.downloadTemporalPixels(pixels.data());
        sutil::Camera moved(make_float3(3.5f, 3, 6.5f), make_float3(0, 0.5f, 0), make_float3(0, 1, 0), 45.0f, scene.fbSize.x / float(scene.fbSize.y));
        sample.setCamera(moved);
        sample.render();
        sample.downloadPixels(pixels.data() + n);
        sample.temporal();
        sample.downloadTemporalPixels(pixels.data() + 2 * n);
        OutFile f(out);
        f.write(pixels.data(), 4, pixels.size());
        f.close();
        // an out-of-range configuration is an exception, like every other error of the shim
        fovpt_temporal_config bad;
        fovpt_temporal_defaults(&bad);
        bad.history_periphery = FOVPT_TEMPORAL_MAX_HISTORY + 1;
        if (!must_throw([&] { sample.temporal(bad); }, text("temporal(history_periphery %d) did not throw", FOVPT_TEMPORAL_MAX_HISTORY + 1))) return 2;
        sample.temporal_reset();
        printf("ok\n");
        return 0;
    });
}
