// Rigid motion through the drop-in C++ API: the box scene of refit_gpu_test.cpp, the red box turned a quarter about the vertical
// axis and carried by SampleRenderer::updateTransforms (a refit), then carried elsewhere from its rest positions with
// rebuild = true; after each, a fresh SampleRenderer over a Model whose vertices went through the same expression renders the
// same frame.  hierarchyCost(true) must come back with measured == updates.  Writes the four rgba8 frames (refit, fresh,
// rebuild, fresh).
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

// the library's expression, one binary32 operation at a time
float row(const float* m, const float3& v)
{
    volatile float a = m[0] * v.x, b = m[1] * v.y, c = m[2] * v.z;
    volatile float ab = a + b;
    volatile float abc = ab + c;
    return abc + m[3];
}

void place(Model* model, const std::vector<float3>& rest, const fovpt_mesh_transform& t)
{
    for (size_t i = 0; i < rest.size(); i++)
        model->meshes[1]->vertex[i] = make_float3(row(t.m, rest[i]), row(t.m + 4, rest[i]), row(t.m + 8, rest[i]));
}
}  // namespace

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "transform_out.bin";
    try {
        Model* model = new Model;
        Material grey; grey.color = make_float3(0.7f, 0.7f, 0.7f); grey.emission = make_float3(0.0f);
        Material red; red.color = make_float3(0.8f, 0.1f, 0.1f); red.emission = make_float3(0.0f);
        addBox(model, grey, make_float3(0, -1.0f, 0), make_float3(6, 0.5f, 6));
        addBox(model, red, make_float3(0, 0.5f, 0), make_float3(1, 2, 0.5f));
        const std::vector<float3> rest = model->meshes[1]->vertex;
        const int2 fbSize = make_int2(160, 96);
        const size_t n = (size_t)fbSize.x * fbSize.y;
        std::vector<float4> sky(n, make_float4(2.5f, 2.5f, 2.5f, 1.0f));
        ProbeData probe;
        probe.width = fbSize.x; probe.height = fbSize.y; probe.data = sky.data();
        probe.BuildCDF();
        std::vector<uint32_t> pixels(n * 4);

        SampleRenderer sample(model);
        setup(sample, probe, fbSize);
        const fovpt_hierarchy_cost_info c0 = sample.hierarchyCost();
        if (c0.updates != 0 || c0.measured != 0 || c0.built != c0.current || !(c0.built >= 1.0)) { printf("cost after the build: %g %g\n", c0.built, c0.current); return 2; }
        // a quarter turn about y (x' = z, z' = -x) with a shear of 0.25 y into x, and a carry
        const fovpt_mesh_transform turn = {1, {0, 0.25f, 1, 0.75f, 0, 1, 0, 0.25f, -1, 0, 0, -0.5f}};
        sample.updateTransforms({turn});
        frame(sample, pixels.data());
        const fovpt_hierarchy_cost_info c1 = sample.hierarchyCost(true);
        if (c1.updates != 1 || c1.measured != c1.updates) { printf("cost after the refit: updates %llu measured %llu\n", (unsigned long long)c1.updates, (unsigned long long)c1.measured); return 2; }
        place(model, rest, turn);
        {
            SampleRenderer fresh(model);
            setup(fresh, probe, fbSize);
            frame(fresh, pixels.data() + n);
        }
        // absolute: from the rest positions again, not from the turned ones
        const fovpt_mesh_transform carry = {1, {1, 0, 0, -1.5f, 0, 1.5f, 0, 0, 0, 0, 1, 0.75f}};
        sample.updateTransforms({carry}, true);
        frame(sample, pixels.data() + 2 * n);
        const fovpt_hierarchy_cost_info c2 = sample.hierarchyCost(true);
        if (c2.updates != 2 || c2.measured != c2.updates || c2.built != c2.current) { printf("cost after the rebuild: updates %llu measured %llu\n", (unsigned long long)c2.updates, (unsigned long long)c2.measured); return 2; }
        place(model, rest, carry);
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
        const fovpt_mesh_transform bad = {2, {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
        try { sample.updateTransforms({bad}); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { printf("updateTransforms of mesh 2 did not throw\n"); return 2; }
        printf("ok\n");
        delete model;
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
