// fovpt_warp_motion through the drop-in C++ API: the box scene of box_scene.h rendered and stepped with SampleRenderer::post(),
// the box carried by updateTransforms(), rendered and stepped again and exposed; then the exposed frame warped to a moved camera with
// warpMotionExposed() -- once tracing its own G-buffer, once with the post step's (reuse_gbuffer) --, the raw frame with a
// fovpt_warp_motion_config (rgba8 only, fill_radius 0, advance 2.5), and the exposed frame with warpExposed() for comparison.  Writes
// the four rgba8 frames and the four counts records to a file.
#include <cstdio>
#include <cstring>
#include <vector>
#include "box_scene.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "warp_motion_out.bin";
    return run_main([&]() -> int {
        BoxScene scene;
        const size_t n = scene.n;
        sutil::Camera moved(make_float3(3.5f, 3, 6.5f), make_float3(0, 0.5f, 0), make_float3(0, 1, 0), 45.0f, 1.0f);   // (the warp sets the aspect ratio)

        SampleRenderer sample(scene.model);
        scene.setup(sample, true);
        std::vector<uint32_t> pixels(n * 4);
        struct fovpt_warp_counts counts[4];
        sample.render();
        // before any temporal step the call is an exception, like every other error of the shim
        if (!must_throw([&] { sample.warpMotion(moved, 1.0f); }, "warpMotion before any temporal step did not throw")) return 2;
        sample.post();
        fovpt_mesh_transform carry;
        carry.mesh = 1;
        const float m[12] = {1, 0, 0, 0.5f, 0, 1, 0, 0.0f, 0, 0, 1, -0.25f};
        memcpy(carry.m, m, sizeof(m));
        sample.updateTransforms(std::vector<fovpt_mesh_transform>(1, carry));
        sample.render();
        sample.post();
        fovpt_expose_config ec;
        if (fovpt_expose_defaults(&ec) != FOVPT_OK) { printf("fovpt_expose_defaults failed\n"); return 2; }
        sample.exposePost(ec);
        sample.warpMotionExposed(moved, 1.0f);
        sample.downloadWarpedPixels(pixels.data());
        counts[0] = sample.warpCounts();
        sample.warpMotionExposed(moved, 1.0f, true);
        sample.downloadWarpedPixels(pixels.data() + n);
        counts[1] = sample.warpCounts();
        if (memcmp(pixels.data(), pixels.data() + n, n * 4) != 0 || memcmp(&counts[0], &counts[1], sizeof(counts[0])) != 0) {
            printf("the post step's G-buffer gives another warp than the call's own trace\n");
            return 2;
        }
        fovpt_warp_motion_config mc;
        if (fovpt_warp_motion_defaults(&mc) != FOVPT_OK) { printf("fovpt_warp_motion_defaults failed\n"); return 2; }
        mc.images = FOVPT_WARP_RGBA; mc.fill_radius = 0; mc.advance = 2.5f;
        sample.warpMotion(moved, mc);
        sample.downloadWarpedPixels(pixels.data() + 2 * n);
        counts[2] = sample.warpCounts();
        if (counts[2].filled != 0) { printf("fill_radius 0 filled pixels\n"); return 2; }
        sample.warpExposed(moved);
        sample.downloadWarpedPixels(pixels.data() + 3 * n);
        counts[3] = sample.warpCounts();
        if (memcmp(pixels.data(), pixels.data() + 3 * n, n * 4) == 0) { printf("the moved box is warped as fovpt_warp warps it\n"); return 2; }
        OutFile f(out);
        f.write(pixels.data(), 4, pixels.size());
        f.write(counts, sizeof(counts[0]), 4);
        f.close();
        mc.advance = FOVPT_WARP_MAX_ADVANCE * 2.0f;
        if (!must_throw([&] { sample.warpMotion(moved, mc); }, text("warpMotion(advance %g) did not throw", (double)mc.advance))) return 2;
        printf("ok\n");
        return 0;
    });
}
