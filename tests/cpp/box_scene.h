// What the drop-in programs of this directory (*_gpu_test.cpp, rccl_gather_test.cpp) share: the scene they render, the set-up
// of a SampleRenderer over it, main's frame, the writer of the file the python side parses and the "this must throw" check.
// tests/gpu_common.py: dropin_renderer() is the python twin of the scene and the set-up; keep the two equal.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>
#include "SimplePathtracer.h"

// A grey slab and a red box under a constant sky of 2.5, seen from (4, 3, 6) at 45 degrees in a 160 x 96 frame.  Owns the model
// and the sky's texels.  red_half: the red box's half extents; `other` (owned from here on) replaces the two boxes.
struct BoxScene {
    const int2 fbSize = make_int2(160, 96);
    const size_t n = (size_t)fbSize.x * fbSize.y;
    Model* const model;
    std::vector<float4> sky;
    ProbeData probe;
    const sutil::Camera camera;

    explicit BoxScene(const float3& red_half = make_float3(1, 1, 1), Model* other = nullptr)
        : model(other ? other : new Model), sky(n, make_float4(2.5f, 2.5f, 2.5f, 1.0f)),
          camera(make_float3(4, 3, 6), make_float3(0, 0.5f, 0), make_float3(0, 1, 0), 45.0f, fbSize.x / float(fbSize.y))
    {
        if (!other) {
            Material grey; grey.color = make_float3(0.7f, 0.7f, 0.7f); grey.emission = make_float3(0.0f);
            Material red; red.color = make_float3(0.8f, 0.1f, 0.1f); red.emission = make_float3(0.0f);
            addBox(model, grey, make_float3(0, -1.0f, 0), make_float3(6, 0.5f, 6));
            addBox(model, red, make_float3(0, 0.5f, 0), red_half);
        }
        probe.width = fbSize.x; probe.height = fbSize.y; probe.data = sky.data();
        probe.BuildCDF();
    }
    ~BoxScene() { delete model; }
    BoxScene(const BoxScene&) = delete;
    BoxScene& operator=(const BoxScene&) = delete;

    // Frame size, camera, probe (other_probe in place of the sky, if given), radii 12 / 36 at 1 / 2 / 8 samples, the gaze at the
    // centre, subframe 0.  `more` sets what else the program wants in the configuration before it is applied.  A program that
    // renders at another gaze or subframe writes it into launchParams after this call, before it renders.  (Some programs used
    // not to set a gaze or a subframe in their set-up: those wrote the gaze before every render, as they still do, and
    // rendered at LaunchParams' default subframe, which is the 0 set here; so the bytes they write are the same.)
    void setup(SampleRenderer& s, bool write_guides = false, const std::function<void(fovpt_config&)>& more = nullptr,
               const ProbeData* other_probe = nullptr) const
    {
        s.resize(fbSize);
        s.setCamera(camera);
        s.setProbe(other_probe ? *other_probe : probe);
        fovpt_config cfg = s.config();
        cfg.r_inner = 12; cfg.r_outer = 36; cfg.spp_periphery = 1; cfg.spp_middle = 2; cfg.spp_fovea = 8;
        if (write_guides) cfg.write_guides = 1;
        if (more) more(cfg);
        s.setConfig(cfg);
        s.launchParams.frame.c.x = fbSize.x / 2;
        s.launchParams.frame.c.y = fbSize.y / 2;
        s.launchParams.frame.subframe_index = 0;
    }
};

// main's frame: the body's own exit code, or 1 with the message of whatever std::exception it let through.
template <class Body> int run_main(Body body)
{
    try {
        return body();
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
}

// The file the python side parses.  A file that cannot be opened, a short write or a failing close is a std::runtime_error
// that names the file, so a full disk or a bad path fails the test with a message.
class OutFile {
public:
    explicit OutFile(const char* path) : path_(path), f_(fopen(path, "wb"))
    {
        if (!f_) throw std::runtime_error("cannot open " + path_ + " for writing");
    }
    ~OutFile() { if (f_) fclose(f_); }
    OutFile(const OutFile&) = delete;
    OutFile& operator=(const OutFile&) = delete;
    void write(const void* p, size_t size, size_t count)          // fwrite's arguments
    {
        if (fwrite(p, size, count, f_) != count) throw std::runtime_error("short write to " + path_);
    }
    void close()
    {
        FILE* f = f_;
        f_ = nullptr;
        if (fclose(f) != 0) throw std::runtime_error("cannot finish " + path_);
    }

private:
    std::string path_;
    FILE* f_;
};

// A short message put together as printf would (the compiler checks the arguments against the format).
__attribute__((format(printf, 1, 2))) inline std::string text(const char* format, ...)
{
    char buf[256];
    va_list args;
    va_start(args, format);
    vsnprintf(buf, sizeof(buf), format, args);
    va_end(args);
    return buf;
}

// f() must throw std::runtime_error, as every error of the shim does.  If it does not: prints the message and a new line and
// returns false, for the caller to leave with exit code 2.
template <class F> bool must_throw(F f, const std::string& message)
{
    try { f(); } catch (const std::runtime_error&) { return true; }
    printf("%s\n", message.c_str());
    return false;
}
