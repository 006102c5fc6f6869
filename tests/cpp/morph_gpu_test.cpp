// Morph targets through the drop-in C++ API: the box scene of transform_gpu_test.cpp, the red box with three targets -- a dense
// one that leans the box, a sparse one that lifts its upper vertices, an empty one -- set by SampleRenderer::setMorphs, posed by
// updateMorphed, rendered.  Prints the FNV-1a hashes of the rgba8 frame and of the "scene_vertices" bytes for the python test
// to compare with the same calls through the python wrapper, then poses again with rebuild = true (the hashes must come back
// the same), checks that a pose of zero weights brings back the bytes of the zero pose made first and that an unmorphed mesh is an exception.
#include <cstdio>
#include <vector>
#include "SimplePathtracer.h"

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
    try {
        Model* model = new Model;
        Material grey; grey.color = make_float3(0.7f, 0.7f, 0.7f); grey.emission = make_float3(0.0f);
        Material red; red.color = make_float3(0.8f, 0.1f, 0.1f); red.emission = make_float3(0.0f);
        addBox(model, grey, make_float3(0, -1.0f, 0), make_float3(6, 0.5f, 6));
        addBox(model, red, make_float3(0, 0.5f, 0), make_float3(1, 2, 0.5f));
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
        sample.setConfig(cfg);
        sample.launchParams.frame.c.x = fbSize.x / 2;
        sample.launchParams.frame.c.y = fbSize.y / 2;

        const std::vector<float3>& v = model->meshes[1]->vertex;
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
        bool threw = false;
        const fovpt_morph_pose bad = {0, 3, weights, 0, 0, nullptr};       // mesh 0 has no morph targets
        try { sample.updateMorphed({bad}); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { printf("updateMorphed of an unmorphed mesh did not throw\n"); return 2; }
        fovpt_mesh_morph none = {1, (uint32_t)v.size(), 0, 0, nullptr};
        sample.setMorphs({none});
        threw = false;
        try { sample.updateMorphed({pose}); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { printf("updateMorphed after the targets were removed did not throw\n"); return 2; }
        printf("ok\n");
        delete model;
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
