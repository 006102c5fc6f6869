// The background rebuild through the drop-in C++ API: the box scene of box_scene.h; the red box moved with
// updateAccel({1}, REBUILD_ASYNC), rebuildState(true) until the new hierarchy is READY, a frame over the refit tree,
// rebuildState(false, true) to adopt, a frame over the adopted one, then another move by a plain refit and a last frame.  Writes
// the four rgba8 frames (rest, refit tree, adopted tree, second move).
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
}  // namespace

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "rebuild_async_out.bin";
    return run_main([&]() -> int {
        BoxScene scene;
        const size_t n = scene.n;

        SampleRenderer sample(scene.model);
        scene.setup(sample);
        std::vector<uint32_t> pixels(n * 4);
        const fovpt_rebuild_info s0 = sample.rebuildState();
        if (s0.state != FOVPT_REBUILD_IDLE || s0.requested != 0) { printf("state before any request: %d\n", s0.state); return 2; }
        frame(sample, pixels.data());
        for (float3& v : scene.model->meshes[1]->vertex) { v.x += 0.5f; v.z -= 0.25f; }
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
        for (float3& v : scene.model->meshes[1]->vertex) { v.x -= 1.0f; v.y += 0.25f; v.z += 0.5f; }
        sample.updateAccel({1});
        frame(sample, pixels.data() + 3 * n);
        OutFile f(out);
        f.write(pixels.data(), 4, pixels.size());
        f.close();
        // both kinds of rebuild at once are refused
        if (fovpt_update_vertices(sample.context(), nullptr, 0, FOVPT_UPDATE_REBUILD | FOVPT_UPDATE_REBUILD_ASYNC) != FOVPT_E_INVALID) {
            printf("both rebuild flags were not refused\n");
            return 2;
        }
        printf("ok\n");
        return 0;
    });
}
