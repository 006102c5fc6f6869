// The post-frame chain through the drop-in C++ API: the box scene of box_scene.h rendered and stepped with
// SampleRenderer::post(), then the red box moved with updateAccel({1}), a second frame and a second post() that also writes
// motion vectors.  Writes the two steps' rgba8 frames and the motion vectors (float4 per pixel) to a file.
#include <cstdio>
#include <vector>
#include "box_scene.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "post_out.bin";
    return run_main([&]() -> int {
        BoxScene scene;
        const size_t n = scene.n;

        SampleRenderer sample(scene.model);
        scene.setup(sample, true);
        std::vector<uint32_t> pixels(n * 2);
        std::vector<float4> motion(n);
        sample.render();
        sample.post();
        sample.downloadPostPixels(pixels.data());
        for (float3& v : scene.model->meshes[1]->vertex) { v.x += 0.5f; v.z -= 0.25f; }
        sample.updateAccel({1});
        sample.render();
        // a float4 frame on the device for the motion vectors: the renderer's normal guide, which the chain does not read
        fovpt_float4* d_motion = reinterpret_cast<fovpt_float4*>(sample.launchParams.frame.normal_buffer);
        fovpt_post_config pc;
        if (fovpt_post_defaults(&pc) != FOVPT_OK) { printf("fovpt_post_defaults failed\n"); return 2; }
        sample.post(pc, nullptr, d_motion);
        sample.downloadPostPixels(pixels.data() + n);
        sample.downloadMotion(d_motion, motion.data());
        OutFile f(out);
        f.write(pixels.data(), 4, pixels.size());
        f.write(motion.data(), sizeof(float4), motion.size());
        f.close();
        // motion vectors need the motion stage
        pc.stages = FOVPT_POST_RECONSTRUCT | FOVPT_POST_TEMPORAL;
        if (!must_throw([&] { sample.post(pc, nullptr, d_motion); }, "post(out_motion without FOVPT_POST_MOTION) did not throw")) return 2;
        printf("ok\n");
        return 0;
    });
}
