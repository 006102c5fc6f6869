// The background rebuild through the drop-in C++ API: the box scene of temporal_motion_gpu_test.cpp; the red box moved with
// updateAccel({1}, REBUILD_ASYNC), rebuildState(true) until the new hierarchy is READY, a frame over the refit tree,
// rebuildState(false, true) to adopt, a frame over the adopted one, then another move by a plain refit and a last frame.  Writes
// the four rgba8 frames (rest, refit tree, adopted tree, second move).
#include <cstdio>
#include <vector>
#include "SimplePathtracer.h"

namespace {
void frame(SampleRenderer& s, uint32_t* out)
{
    s.launchParams.frame.subframe_index = 0;
    s.render();
    s.downloadPixels(out);
}
}  // namespace

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "rebuild_async_out.bin";
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
        sample.setConfig(cfg);
        sample.launchParams.frame.c.x = fbSize.x / 2;
        sample.launchParams.frame.c.y = fbSize.y / 2;
        std::vector<uint32_t> pixels(n * 4);
        const fovpt_rebuild_info s0 = sample.rebuildState();
        if (s0.state != FOVPT_REBUILD_IDLE || s0.requested != 0) { printf("state before any request: %d\n", s0.state); return 2; }
        frame(sample, pixels.data());
        for (float3& v : model->meshes[1]->vertex) { v.x += 0.5f; v.z -= 0.25f; }
        sample.updateAccel({1}, SampleRenderer::REBUILD_ASYNC);
        const fovpt_rebuild_info s1 = sample.rebuildState(true);
        if (s1.state != FOVPT_REBUILD_READY || s1.requested != 1 || s1.started != 1 || s1.adopted != 0 || s1.snapshot_update != 1) {
            printf("after the wait: state %d, requested %llu, started %llu\n", s1.state, (unsigned long long)s1.requested, (unsigned long long)s1.started);
            return 2;
        }
        frame(sample, pixels.data() + n);
        const fovpt_rebuild_info s2 = sample.rebuildState(false, true);
        if (s2.state != FOVPT_REBUILD_IDLE || s2.adopted != 1 || s2.failed != 0 || !(s2.ms_build > 0.0)) {
            printf("after the adoption: state %d, adopted %llu, ms %g\n", s2.state, (unsigned long long)s2.adopted, s2.ms_build);
            return 2;
        }
        const fovpt_hierarchy_cost_info c = sample.hierarchyCost(true);
        if (c.updates != 2 || c.measured != 2) { printf("updates %llu after a refit and an adoption\n", (unsigned long long)c.updates); return 2; }
        frame(sample, pixels.data() + 2 * n);
        for (float3& v : model->meshes[1]->vertex) { v.x -= 1.0f; v.y += 0.25f; v.z += 0.5f; }
        sample.updateAccel({1});
        frame(sample, pixels.data() + 3 * n);
        FILE* f = fopen(out, "wb");
        fwrite(pixels.data(), 4, pixels.size(), f);
        fclose(f);
        // both kinds of rebuild at once are refused
        if (fovpt_update_vertices(sample.context(), nullptr, 0, FOVPT_UPDATE_REBUILD | FOVPT_UPDATE_REBUILD_ASYNC) != FOVPT_E_INVALID) {
            printf("both rebuild flags were not refused\n");
            return 2;
        }
        printf("ok\n");
        delete model;
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
