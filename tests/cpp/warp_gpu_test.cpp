// fovpt_warp through the drop-in C++ API: the box scene of box_scene.h rendered, stepped with SampleRenderer::post() and exposed,
// then the exposed frame warped to a moved camera twice -- once tracing its own G-buffer, once with the post step's (reuse_gbuffer)
// -- and the raw frame warped with fill_radius 0.  Writes the three rgba8 frames and the three counts records to a file.
#include <cstdio>
#include <cstring>
#include <vector>
#include "box_scene.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "warp_out.bin";
    return run_main([&]() -> int {
        BoxScene scene;
        const size_t n = scene.n;
        sutil::Camera moved(make_float3(3.5f, 3, 6.5f), make_float3(0, 0.5f, 0), make_float3(0, 1, 0), 45.0f, 1.0f);   // (warp sets the aspect ratio)

        SampleRenderer sample(scene.model);
        scene.setup(sample, true);
        std::vector<uint32_t> pixels(n * 3);
        struct fovpt_warp_counts counts[3];
        struct fovpt_warp_counts none = sample.warpCounts();
        if (none.splatted || none.direct || none.filled || none.empty) { printf("counts before any warp are not zero\n"); return 2; }
        sample.render();
        sample.post();
        fovpt_expose_config ec;
        if (fovpt_expose_defaults(&ec) != FOVPT_OK) { printf("fovpt_expose_defaults failed\n"); return 2; }
        sample.exposePost(ec);
        sample.warpExposed(moved);
        sample.downloadWarpedPixels(pixels.data());
        counts[0] = sample.warpCounts();
        sample.warpExposed(moved, true);
        sample.downloadWarpedPixels(pixels.data() + n);
        counts[1] = sample.warpCounts();
        if (memcmp(pixels.data(), pixels.data() + n, n * 4) != 0 || memcmp(&counts[0], &counts[1], sizeof(counts[0])) != 0) {
            printf("the post step's G-buffer gives another warp than the call's own trace\n");
            return 2;
        }
        fovpt_warp_config wc;
        if (fovpt_warp_defaults(&wc) != FOVPT_OK) { printf("fovpt_warp_defaults failed\n"); return 2; }
        wc.images = FOVPT_WARP_RGBA; wc.fill_radius = 0;
        sample.warp(moved, wc);
        sample.downloadWarpedPixels(pixels.data() + 2 * n);
        counts[2] = sample.warpCounts();
        if (counts[2].filled != 0 || counts[2].direct != counts[0].direct) { printf("fill_radius 0 filled pixels or changed the direct ones\n"); return 2; }
        OutFile f(out);
        f.write(pixels.data(), 4, pixels.size());
        f.write(counts, sizeof(counts[0]), 3);
        f.close();
        // an out-of-range configuration is an exception, like every other error of the shim
        wc.fill_radius = FOVPT_WARP_MAX_RADIUS + 1;
        if (!must_throw([&] { sample.warp(moved, wc); }, text("warp(fill_radius %d) did not throw", FOVPT_WARP_MAX_RADIUS + 1))) return 2;
        printf("ok\n");
        return 0;
    });
}
