// Morph targets through the drop-in C++ API: the tall-box scene of box_scene.h, the red box with three targets -- a dense
// one that leans the box, a sparse one that lifts its upper vertices, an empty one -- set by SampleRenderer::setMorphs, posed by
// updateMorphed, rendered.  Prints the FNV-1a hashes of the rgba8 frame and of the "scene_vertices" bytes for the python test
// to compare with the same calls through the python wrapper, then poses again with rebuild = true (the hashes must come back
// the same), checks that a pose of zero weights brings back the bytes of the zero pose made first and that an unmorphed mesh is an exception.
#include <cstdio>
#include <vector>
#include "box_scene.h"

namespace {
unsigned long long fnv1a(const void* p, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) { h ^= ((const unsigned char*)p)[i]; h *= 1099511628211ull; }
    return h;
}

unsigned long long vertex_hash(SampleRenderer& s)
{
    void* p = nullptr;
    size_t bytes = 0;
    if (fovpt_debug_buffer(s.context(), "scene_vertices", &p, &bytes) != FOVPT_OK) throw std::runtime_error("no scene_vertices buffer");
    std::vector<unsigned char> h(bytes);
    if (fovpt_synchronize(s.context()) != FOVPT_OK || fovpt_download(s.context(), p, h.data(), bytes) != FOVPT_OK) throw std::runtime_error("download failed");
    return fnv1a(h.data(), bytes);
}

unsigned long long frame_hash(SampleRenderer& s, std::vector<uint32_t>& pixels)
{
    s.launchParams.frame.subframe_index = 0;
    s.render();
    s.downloadPixels(pixels.data());
    return fnv1a(pixels.data(), pixels.size() * 4);
}
}  // namespace

int main()
{
    return run_main([&]() -> int {
        BoxScene scene(make_float3(1, 2, 0.5f));
        const size_t n = scene.n;
        SampleRenderer sample(scene.model);
        scene.setup(sample);

        const std::vector<float3>& v = scene.model->meshes[1]->vertex;
        std::vector<float> lean(3 * v.size(), 0.0f), lift;
        std::vector<uint32_t> upper;
        for (size_t i = 0; i < v.size(); i++) {
            lean[3 * i] = 0.25f * v[i].y;
            lean[3 * i + 2] = -0.125f;
            if (v[i].y > 0.5f) { upper.push_back((uint32_t)i); lift.push_back(0.0f); lift.push_back(0.5f); lift.push_back(0.0625f * (float)(i % 3)); }
        }
        const fovpt_morph_target targets[3] = {{(uint32_t)v.size(), 0, nullptr, lean.data()},
                                               {(uint32_t)upper.size(), 0, upper.data(), lift.data()},
                                               {0, 0, nullptr, nullptr}};
        fovpt_mesh_morph morph = {1, (uint32_t)v.size(), 3, 0, targets};
        sample.setMorphs({morph});
        const float weights[3] = {1.5f, -0.75f, 2.0f};
        const fovpt_morph_pose pose = {1, 3, weights, 0, 0, nullptr};
        const float zeros[3] = {0.0f, -0.0f, 0.0f};
        const fovpt_morph_pose at_rest = {1, 3, zeros, 0, 0, nullptr};
        sample.updateMorphed({at_rest});                                    // (the first update makes the "scene_vertices" buffer)
        const unsigned long long v0 = vertex_hash(sample);
        std::vector<uint32_t> pixels(n);
        sample.updateMorphed({pose});
        const unsigned long long f1 = frame_hash(sample, pixels), v1 = vertex_hash(sample);
        printf("frame %016llx vertices %016llx\n", f1, v1);
        sample.updateMorphed({pose}, true);
        const unsigned long long f2 = frame_hash(sample, pixels), v2 = vertex_hash(sample);
        if (f1 != f2 || v1 != v2) { printf("rebuild: frame %016llx vertices %016llx\n", f2, v2); return 2; }
        sample.updateMorphed({at_rest});
        if (vertex_hash(sample) != v0 || v1 == v0) { printf("a pose of zero weights did not bring the rest positions back\n"); return 2; }
        const fovpt_morph_pose bad = {0, 3, weights, 0, 0, nullptr};       // mesh 0 has no morph targets
        if (!must_throw([&] { sample.updateMorphed({bad}); }, "updateMorphed of an unmorphed mesh did not throw")) return 2;
        fovpt_mesh_morph none = {1, (uint32_t)v.size(), 0, 0, nullptr};
        sample.setMorphs({none});
        if (!must_throw([&] { sample.updateMorphed({pose}); }, "updateMorphed after the targets were removed did not throw")) return 2;
        printf("ok\n");
        return 0;
    });
}
