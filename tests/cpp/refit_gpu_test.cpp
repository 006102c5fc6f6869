// Animated geometry through the drop-in C++ API: the box scene of box_scene.h, the red box moved in the Model and
// SampleRenderer::updateAccel({1}) (a refit), then moved again and updateAccel({1}, true) (a rebuild); after each, a fresh
// SampleRenderer over the mutated Model renders the same frame.  Writes the four rgba8 frames (refit, fresh, rebuild, fresh).
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

void move(Model* model, float dx, float dy, float dz)
{
    for (float3& v : model->meshes[1]->vertex) { v.x += dx; v.y += dy; v.z += dz; }
}
}  // namespace

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "refit_out.bin";
    return run_main([&]() -> int {
        BoxScene scene;
        const size_t n = scene.n;
        std::vector<uint32_t> pixels(n * 4);

        SampleRenderer sample(scene.model);
        scene.setup(sample);
        frame(sample, pixels.data());
        move(scene.model, 0.75f, 0.25f, -0.5f);
        sample.updateAccel({1});
        frame(sample, pixels.data());
        {
            SampleRenderer fresh(scene.model);
            scene.setup(fresh);
            frame(fresh, pixels.data() + n);
        }
        move(scene.model, -1.5f, 0.0f, 0.75f);
        sample.updateAccel({1}, true);
        frame(sample, pixels.data() + 2 * n);
        {
            SampleRenderer fresh(scene.model);
            scene.setup(fresh);
            frame(fresh, pixels.data() + 3 * n);
        }
        OutFile f(out);
        f.write(pixels.data(), 4, pixels.size());
        f.close();
        // an out-of-range mesh is an exception, like every other error of the shim
        if (!must_throw([&] { sample.updateAccel({2}); }, "updateAccel({2}) did not throw")) return 2;
        printf("ok\n");
        return 0;
    });
}
