// A rig through the drop-in C++ API: the tall-box scene of box_scene.h, the red box skinned over two joints that are nodes 0 and
// 1 of a rig (node 1 turning about z on node 0, which scales), the floor rigid on node 2 (which drops by STEP).
// SampleRenderer::setRig uploads it, updateAnimated poses it at t = 0.75.  Prints the FNV-1a hashes of the rgba8 frame and of the
// "scene_vertices" bytes for the python test to compare with the same calls through the python wrapper, then poses again with
// rebuild = true (the hashes must come back the same) and checks that a clip out of range, a removed rig and a rig dropped by
// setSkins are exceptions.
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

        const fovpt_rig_node nodes[3] = {{-1, {0, -0.5f, 0}, {0, 0, 0, 1}, {1, 1, 1}}, {0, {0, 2, 0}, {0, 0, 0, 1}, {1, 1, 1}}, {-1, {0, 0, 0}, {0, 0, 0, 1}, {1, 1, 1}}};
        const uint16_t joint_nodes[2] = {0, 1};
        const float inverse_bind[24] = {1, 0, 0, 0, 0, 1, 0, 0.5f, 0, 0, 1, 0,
                                        1, 0, 0, 0, 0, 1, 0, -1.5f, 0, 0, 1, 0};
        const fovpt_rig_binding bindings[2] = {{1, -1, 2, 0, joint_nodes, inverse_bind}, {0, 2, 0, 0, nullptr, nullptr}};
        const float t01[2] = {0.0f, 1.0f}, t02[2] = {0.0f, 2.0f};
        const float turn[8] = {0, 0, 0, 1, 0, 0, 0.5f, 0.8660254f};
        const float scale[6] = {1, 1, 1, 1.5f, 1, 0.5f};
        const float drop[6] = {0, 0, 0, 0, -0.25f, 0};
        const fovpt_rig_channel channels[3] = {{1, FOVPT_RIG_ROTATION, FOVPT_RIG_LINEAR, 2, t01, turn}, {0, FOVPT_RIG_SCALE, FOVPT_RIG_LINEAR, 2, t02, scale},
                                               {2, FOVPT_RIG_TRANSLATION, FOVPT_RIG_STEP, 2, t01, drop}};
        const fovpt_rig_clip clip = {3, 0, channels};
        const fovpt_rig_desc rig = {nodes, 3, 0, bindings, 2, 0, &clip, 1, 0};
        sample.setRig(&rig);

        std::vector<uint32_t> pixels(n);
        sample.updateAnimated(0, 0.75f);
        const unsigned long long f1 = frame_hash(sample, pixels), v1 = vertex_hash(sample);
        printf("frame %016llx vertices %016llx\n", f1, v1);
        sample.updateAnimated(0, 0.75f, true);
        const unsigned long long f2 = frame_hash(sample, pixels), v2 = vertex_hash(sample);
        if (f1 != f2 || v1 != v2) { printf("rebuild: frame %016llx vertices %016llx\n", f2, v2); return 2; }
        if (!must_throw([&] { sample.updateAnimated(1, 0.0f); }, "a clip out of range did not throw")) return 2;
        sample.setRig(nullptr);
        if (!must_throw([&] { sample.updateAnimated(0, 0.0f); }, "updateAnimated after the rig was removed did not throw")) return 2;
        sample.setRig(&rig);
        sample.updateAnimated(0, 0.75f);
        if (vertex_hash(sample) != v1) { printf("the rig set again poses differently\n"); return 2; }
        sample.setSkins({skin});
        if (!must_throw([&] { sample.updateAnimated(0, 0.0f); }, "updateAnimated after setSkins did not throw")) return 2;
        printf("ok\n");
        return 0;
    });
}
