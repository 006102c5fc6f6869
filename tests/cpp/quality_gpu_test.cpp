// fovpt_quality through the drop-in C++ API: the box scene of box_scene.h rendered foveated, its frame buffer measured against
// the lens stage's rgba8 image of the same frame (another image of the frame's size that lives on the device) with
// SampleRenderer::measureQuality(), then the other way round with a configuration of the caller's, then the frame buffer against
// itself through qualityAsync() / readQuality().  Writes the three records to a file.
#include <cstdio>
#include <cstring>
#include <vector>
#include "box_scene.h"

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "quality_out.bin";
    return run_main([&]() -> int {
        BoxScene scene;
        const size_t n = scene.n;

        SampleRenderer sample(scene.model);
        scene.setup(sample);
        sample.launchParams.frame.c.x = scene.fbSize.x / 2 + 30;
        sample.launchParams.frame.c.y = scene.fbSize.y / 2 - 10;
        sample.render();
        sample.lens();
        fovpt_float4* lens_color = nullptr;
        uint32_t* lens_rgba = nullptr;
        sample.lensBuffers(&lens_color, &lens_rgba);
        const uint32_t* frame = (const uint32_t*)sample.launchParams.frame.frame_buffer;

        fovpt_quality_sums s[3];
        s[0] = sample.measureQuality(lens_rgba);                                   // the frame buffer against the lens image, the defaults
        fovpt_quality_config qc = SampleRenderer::qualityDefaults();
        if (qc.flags != (FOVPT_QUALITY_SSIM | FOVPT_QUALITY_PROFILE) || qc.ring_width != 16) { printf("unexpected defaults\n"); return 2; }
        qc.flags = FOVPT_QUALITY_PROFILE; qc.ring_width = 5;
        s[1] = sample.measureQuality(frame, lens_rgba, &qc);
        sample.qualityAsync(frame, frame);
        s[2] = sample.readQuality();
        if (s[0].width != 160u || s[0].height != 96u || s[1].ring_width != 5u || s[1].flags != 2u) { printf("the header fields do not echo the call\n"); return 2; }
        if (fovpt_quality_mse(&s[2], -1) != 0.0 || !(fovpt_quality_mse(&s[0], -1) > 0.0) || fovpt_quality_ssim(&s[2], -1) != 1.0) { printf("unexpected scores\n"); return 2; }
        // unknown flag bits are refused, and the renderer's record stays
        qc.flags = 4;
        if (!must_throw([&] { sample.measureQuality(frame, lens_rgba, &qc); }, "measureQuality(flags 4) did not throw")) return 2;
        const fovpt_quality_sums again = sample.readQuality();
        if (memcmp(&again, &s[2], sizeof(again)) != 0) { printf("a refused call changed the record\n"); return 2; }
        OutFile f(out);
        f.write(s, sizeof(s[0]), 3);
        f.close();
        printf("ok\n");
        return 0;
    });
}
