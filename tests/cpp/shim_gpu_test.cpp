// Uses the drop-in C++ API the way PT_sv5_/main.cpp:297-306,423 does, on the box scene of box_scene.h
// (or, with a second argument, on the OBJ file it names, through loadOBJ), and writes the rgba8 frame to a file
// for the python test to compare with the oracle.
#include <cstdio>
#include <vector>
#include "box_scene.h"

struct HostTarget {                      // stands in for sutil::CUDAOutputBuffer<uint32_t>
    uint32_t* dev;
    uint32_t* map() { return dev; }
    void unmap() {}
};

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "shim_out.bin";
    return run_main([&]() -> int {
        BoxScene scene(make_float3(1, 1, 1), argc > 2 ? loadOBJ(argv[2]) : nullptr);   // main.cpp:130-145: the scene from an OBJ file
        ProbeData loaded;                             // loadProbe, main.cpp:160-171, without stb_image; else loadColor, :175-187
        if (argc > 3) {
            float4* data = nullptr;
            int resX = 0, resY = 0;
            if (fovpt_image_load_float4(argv[3], &resX, &resY, (fovpt_float4**)&data)) throw std::runtime_error(fovpt_last_error(nullptr));
            loaded.width = resX; loaded.height = resY; loaded.data = data;
            loaded.BuildCDF();
        }

        SampleRenderer sample(scene.model);
        scene.setup(sample, false, nullptr, argc > 3 ? &loaded : nullptr);
        sample.render();
        std::vector<uint32_t> pixels(scene.n);
        sample.downloadPixels(pixels.data());
        OutFile f(out);
        f.write(pixels.data(), 4, pixels.size());
        f.close();
        printf("ok subframe_index=%u\n", sample.launchParams.frame.subframe_index);
        if (!must_throw([&] { ProbeData bad; sample.setProbe(bad); }, "setProbe(invalid) did not throw")) return 2;
        return 0;
    });
}
