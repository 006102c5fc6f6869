// fovpt_warp through the drop-in C++ API: the box scene of post_gpu_test.cpp rendered, stepped with SampleRenderer::post() and exposed,
// then the exposed frame warped to a moved camera twice -- once tracing its own G-buffer, once with the post step's (reuse_gbuffer)
// -- and the raw frame warped with fill_radius 0.  Writes the three rgba8 frames and the three counts records to a file.
#include <cstdio>
#include <cstring>
#include <vector>
#include "SimplePathtracer.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "warp_out.bin";
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
        sutil::Camera moved(make_float3(3.5f, 3, 6.5f), make_float3(0, 0.5f, 0), make_float3(0, 1, 0), 45.0f, 1.0f);   // (warp sets the aspect ratio)

        SampleRenderer sample(model);
        sample.resize(fbSize);
        sample.setCamera(camera);
        sample.setProbe(probe);
        fovpt_config cfg = sample.config();
        cfg.r_inner = 12; cfg.r_outer = 36; cfg.spp_periphery = 1; cfg.spp_middle = 2; cfg.spp_fovea = 8;
        cfg.write_guides = 1;
        sample.setConfig(cfg);
        sample.launchParams.frame.c.x = fbSize.x / 2;
        sample.launchParams.frame.c.y = fbSize.y / 2;
        sample.launchParams.frame.subframe_index = 0;
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
        FILE* f = fopen(out, "wb");
        fwrite(pixels.data(), 4, pixels.size(), f);
        fwrite(counts, sizeof(counts[0]), 3, f);
        fclose(f);
        // an out-of-range configuration is an exception, like every other error of the shim
        bool threw = false;
        wc.fill_radius = FOVPT_WARP_MAX_RADIUS + 1;
        try { sample.warp(moved, wc); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { printf("warp(fill_radius %d) did not throw\n", FOVPT_WARP_MAX_RADIUS + 1); return 2; }
        printf("ok\n");
        delete model;
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
