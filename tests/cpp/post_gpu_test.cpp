// The post-frame chain through the drop-in C++ API: the box scene of temporal_motion_gpu_test.cpp rendered and stepped with
// SampleRenderer::post(), then the red box moved with updateAccel({1}), a second frame and a second post() that also writes
// motion vectors.  Writes the two steps' rgba8 frames and the motion vectors (float4 per pixel) to a file.
#include <cstdio>
#include <vector>
#include "SimplePathtracer.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "post_out.bin";
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
        cfg.write_guides = 1;
        sample.setConfig(cfg);
        sample.launchParams.frame.c.x = fbSize.x / 2;
        sample.launchParams.frame.c.y = fbSize.y / 2;
        sample.launchParams.frame.subframe_index = 0;
        std::vector<uint32_t> pixels(n * 2);
        std::vector<float4> motion(n);
        sample.render();
        sample.post();
        sample.downloadPostPixels(pixels.data());
        for (float3& v : model->meshes[1]->vertex) { v.x += 0.5f; v.z -= 0.25f; }
        sample.updateAccel({1});
        sample.render();
        // a float4 frame on the device for the motion vectors: the renderer's normal guide, which the chain does not read
        fovpt_float4* d_motion = reinterpret_cast<fovpt_float4*>(sample.launchParams.frame.normal_buffer);
        fovpt_post_config pc;
        if (fovpt_post_defaults(&pc) != FOVPT_OK) { printf("fovpt_post_defaults failed\n"); return 2; }
        sample.post(pc, nullptr, d_motion);
        sample.downloadPostPixels(pixels.data() + n);
        sample.downloadMotion(d_motion, motion.data());
        FILE* f = fopen(out, "wb");
        fwrite(pixels.data(), 4, pixels.size(), f);
        fwrite(motion.data(), sizeof(float4), motion.size(), f);
        fclose(f);
        // motion vectors need the motion stage
        bool threw = false;
        pc.stages = FOVPT_POST_RECONSTRUCT | FOVPT_POST_TEMPORAL;
        try { sample.post(pc, nullptr, d_motion); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { printf("post(out_motion without FOVPT_POST_MOTION) did not throw\n"); return 2; }
        printf("ok\n");
        delete model;
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
