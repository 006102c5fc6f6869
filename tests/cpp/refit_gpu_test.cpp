// Animated geometry through the drop-in C++ API: the box scene of shim_gpu_test.cpp, the red box moved in the Model and
// SampleRenderer::updateAccel({1}) (a refit), then moved again and updateAccel({1}, true) (a rebuild); after each, a fresh
// SampleRenderer over the mutated Model renders the same frame.  Writes the four rgba8 frames (refit, fresh, rebuild, fresh).
#include <cstdio>
#include <vector>
#include "SimplePathtracer.h"

namespace {
void setup(SampleRenderer& s, const ProbeData& probe, const int2 fbSize)
{
    sutil::Camera camera(make_float3(4, 3, 6), make_float3(0, 0.5f, 0), make_float3(0, 1, 0), 45.0f, fbSize.x / float(fbSize.y));
    s.resize(fbSize);
    s.setCamera(camera);
    s.setProbe(probe);
    fovpt_config cfg = s.config();
    cfg.r_inner = 12; cfg.r_outer = 36; cfg.spp_periphery = 1; cfg.spp_middle = 2; cfg.spp_fovea = 8;
    s.setConfig(cfg);
    s.launchParams.frame.c.x = fbSize.x / 2;
    s.launchParams.frame.c.y = fbSize.y / 2;
}

void frame(SampleRenderer& s, uint32_t* out)
{
    s.launchParams.frame.subframe_index = 0;
    s.render();
    s.downloadPixels(out);
}

void move(Model* model, float dx, float dy, float dz)
{
    for (float3& v : model->meshes[1]->vertex) { v.x += dx; v.y += dy; v.z += dz; }
}
}  // namespace

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "refit_out.bin";
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
        std::vector<uint32_t> pixels(n * 4);

        SampleRenderer sample(model);
        setup(sample, probe, fbSize);
        frame(sample, pixels.data());
        move(model, 0.75f, 0.25f, -0.5f);
        sample.updateAccel({1});
        frame(sample, pixels.data());
        {
            SampleRenderer fresh(model);
            setup(fresh, probe, fbSize);
            frame(fresh, pixels.data() + n);
        }
        move(model, -1.5f, 0.0f, 0.75f);
        sample.updateAccel({1}, true);
        frame(sample, pixels.data() + 2 * n);
        {
            SampleRenderer fresh(model);
            setup(fresh, probe, fbSize);
            frame(fresh, pixels.data() + 3 * n);
        }
        FILE* f = fopen(out, "wb");
        fwrite(pixels.data(), 4, pixels.size(), f);
        fclose(f);
        // an out-of-range mesh is an exception, like every other error of the shim
        bool threw = false;
        try { sample.updateAccel({2}); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { printf("updateAccel({2}) did not throw\n"); return 2; }
        printf("ok\n");
        delete model;
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
