// Skinning through the drop-in C++ API: the tall-box scene of box_scene.h, the red box skinned over two joints (its lower
// vertices on joint 0, its upper ones three quarters on joint 1) by SampleRenderer::setSkins, posed by updateSkinned, rendered.
// Prints the FNV-1a hashes of the rgba8 frame and of the "scene_vertices" bytes for the python test to compare with the same
// calls through the python wrapper, then poses again with rebuild = true (the hashes must come back the same) and checks that an
// unskinned mesh is an exception.
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
        std::vector<uint16_t> joints(4 * v.size(), 0);
        std::vector<float> weights(4 * v.size(), 0.0f);
        for (size_t i = 0; i < v.size(); i++) {
            if (v[i].y > 0.5f) { joints[4 * i + 1] = 1; weights[4 * i] = 0.25f; weights[4 * i + 1] = 0.75f; }
            else weights[4 * i] = 1.0f;
        }
        fovpt_mesh_skin skin = {1, (uint32_t)v.size(), 2, 0, joints.data(), weights.data()};
        sample.setSkins({skin});
        // joint 0 stays; joint 1: a quarter turn about y with a shear of 0.25 y into x, and a carry
        const float palette[24] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0,
                                   0, 0.25f, 1, 0.75f, 0, 1, 0, 0.25f, -1, 0, 0, -0.5f};
        const fovpt_skin_pose pose = {1, 2, palette};
        std::vector<uint32_t> pixels(n);
        sample.updateSkinned({pose});
        const unsigned long long f1 = frame_hash(sample, pixels), v1 = vertex_hash(sample);
        printf("frame %016llx vertices %016llx\n", f1, v1);
        sample.updateSkinned({pose}, true);
        const unsigned long long f2 = frame_hash(sample, pixels), v2 = vertex_hash(sample);
        if (f1 != f2 || v1 != v2) { printf("rebuild: frame %016llx vertices %016llx\n", f2, v2); return 2; }
        const fovpt_skin_pose bad = {0, 2, palette};                       // mesh 0 has no skin
        if (!must_throw([&] { sample.updateSkinned({bad}); }, "updateSkinned of an unskinned mesh did not throw")) return 2;
        fovpt_mesh_skin none = {1, (uint32_t)v.size(), 0, 0, nullptr, nullptr};
        sample.setSkins({none});
        if (!must_throw([&] { sample.updateSkinned({pose}); }, "updateSkinned after the skin was removed did not throw")) return 2;
        printf("ok\n");
        return 0;
    });
}
