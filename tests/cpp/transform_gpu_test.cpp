// Rigid motion through the drop-in C++ API: the tall-box scene of box_scene.h, the red box turned a quarter about the vertical
// axis and carried by SampleRenderer::updateTransforms (a refit), then carried elsewhere from its rest positions with
// rebuild = true; after each, a fresh SampleRenderer over a Model whose vertices went through the same expression renders the
// same frame.  hierarchyCost(true) must come back with measured == updates.  Writes the four rgba8 frames (refit, fresh,
// rebuild, fresh).
#include <cstdio>
#include <vector>
#include "box_scene.h"

namespace {
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
    return run_main([&]() -> int {
        BoxScene scene(make_float3(1, 2, 0.5f));
        const std::vector<float3> rest = scene.model->meshes[1]->vertex;
        const size_t n = scene.n;
        std::vector<uint32_t> pixels(n * 4);

        SampleRenderer sample(scene.model);
        scene.setup(sample);
        const fovpt_hierarchy_cost_info c0 = sample.hierarchyCost();
        if (c0.updates != 0 || c0.measured != 0 || c0.built != c0.current || !(c0.built >= 1.0)) { printf("cost after the build: %g %g\n", c0.built, c0.current); return 2; }
        // a quarter turn about y (x' = z, z' = -x) with a shear of 0.25 y into x, and a carry
        const fovpt_mesh_transform turn = {1, {0, 0.25f, 1, 0.75f, 0, 1, 0, 0.25f, -1, 0, 0, -0.5f}};
        sample.updateTransforms({turn});
        frame(sample, pixels.data());
        const fovpt_hierarchy_cost_info c1 = sample.hierarchyCost(true);
        if (c1.updates != 1 || c1.measured != c1.updates) { printf("cost after the refit: updates %llu measured %llu\n", (unsigned long long)c1.updates, (unsigned long long)c1.measured); return 2; }
        place(scene.model, rest, turn);
        {
            SampleRenderer fresh(scene.model);
            scene.setup(fresh);
            frame(fresh, pixels.data() + n);
        }
        // absolute: from the rest positions again, not from the turned ones
        const fovpt_mesh_transform carry = {1, {1, 0, 0, -1.5f, 0, 1.5f, 0, 0, 0, 0, 1, 0.75f}};
        sample.updateTransforms({carry}, true);
        frame(sample, pixels.data() + 2 * n);
        const fovpt_hierarchy_cost_info c2 = sample.hierarchyCost(true);
        if (c2.updates != 2 || c2.measured != c2.updates || c2.built != c2.current) { printf("cost after the rebuild: updates %llu measured %llu\n", (unsigned long long)c2.updates, (unsigned long long)c2.measured); return 2; }
        place(scene.model, rest, carry);
        {
            SampleRenderer fresh(scene.model);
            scene.setup(fresh);
            frame(fresh, pixels.data() + 3 * n);
        }
        OutFile f(out);
        f.write(pixels.data(), 4, pixels.size());
        f.close();
        // an out-of-range mesh is an exception, like every other error of the shim
        const fovpt_mesh_transform bad = {2, {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
        if (!must_throw([&] { sample.updateTransforms({bad}); }, "updateTransforms of mesh 2 did not throw")) return 2;
        printf("ok\n");
        return 0;
    });
}
