// Depth packets and the client's warp through the drop-in C++ API: the box scene of box_scene.h rendered, its colour and its
// depth submitted as packets (submitPacket, submitDepthPacket: two slots of the same four), both waited for and checked; then the
// client's side from the two packets' bytes alone -- uploaded, decoded on the device (decodePacket, decodeDepthPacket) and warped
// to a moved camera (warpDepth) with the camera the depth packet's header carries.  Writes the two packets, the decoded depth,
// the warped rgba8 image, the map and the counts to a file; the python side redoes all of it with the restatements.
#include <cstdio>
#include <cstring>
#include <vector>
#include "box_scene.h"

// (the HIP runtime calls this program needs, declared by hand: hip_runtime_api.h brings its own float3 / make_float3, which are
// the shim's job here)
extern "C" {
int hipMalloc(void** ptr, size_t size);
int hipFree(void* ptr);
int hipMemset(void* dst, int value, size_t size);
int hipMemcpy(void* dst, const void* src, size_t size, int kind);
}
enum { hipSuccess = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };

static void* device(size_t bytes)
{
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess || hipMemset(p, 0, bytes) != hipSuccess) throw std::runtime_error("hipMalloc");
    return p;
}

int main(int argc, char** argv)
{
    const char* out = argc > 1 ? argv[1] : "packet_depth_out.bin";
    return run_main([&]() -> int {
        BoxScene scene;
        const size_t n = scene.n;
        const int w = scene.fbSize.x, h = scene.fbSize.y;
        sutil::Camera moved(make_float3(3.5f, 3, 6.5f), make_float3(0, 0.5f, 0), make_float3(0, 1, 0), 45.0f, 1.0f);   // (warpCamera sets the aspect ratio)

        SampleRenderer sample(scene.model);
        scene.setup(sample, true);
        sample.render();
        const int sc = sample.submitPacket(7u), sd = sample.submitDepthPacket(8u);
        if (sc != 0 || sd != 1) { printf("the submits used slots %d and %d\n", sc, sd); return 2; }
        const SampleRenderer::Packet pc = sample.waitPacket(sc), pd = sample.waitPacket(sd);
        fovpt_packet_header hc;
        fovpt_packet_depth_header hd;
        memcpy(&hc, pc.data, sizeof(hc));
        memcpy(&hd, pd.data, sizeof(hd));
        if (fovpt_packet_check(pc.data, pc.bytes) != FOVPT_OK || hc.sequence != 7u) { printf("the colour packet is not valid\n"); return 2; }
        if (fovpt_packet_check_depth(pd.data, pd.bytes) != FOVPT_OK || hd.base.sequence != 8u || hd.base.bytes != pd.bytes || hd.base.npass != hc.npass) {
            printf("the depth packet is not valid\n");
            return 2;
        }
        if (fovpt_packet_check(pd.data, pd.bytes) == FOVPT_OK || fovpt_packet_check_depth(pc.data, pc.bytes) == FOVPT_OK) { printf("a check took the other kind of packet\n"); return 2; }
        if (pd.bytes >= pc.bytes) { printf("the depth packet (%zu bytes) is not smaller than the colour packet (%zu)\n", pd.bytes, pc.bytes); return 2; }
        std::vector<unsigned char> colour((const unsigned char*)pc.data, (const unsigned char*)pc.data + pc.bytes);
        std::vector<unsigned char> deep((const unsigned char*)pd.data, (const unsigned char*)pd.data + pd.bytes);

        // the client: the bytes, a depth image, an rgba8 image and the warp's outputs on the device
        void* dev_colour = device(colour.size());
        void* dev_deep = device(deep.size());
        float* depth = (float*)device(n * 4);
        uint32_t *rgba = (uint32_t*)device(n * 4), *warped = (uint32_t*)device(n * 4), *map = (uint32_t*)device(n * 4);
        if (hipMemcpy(dev_colour, colour.data(), colour.size(), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dev_deep, deep.data(), deep.size(), hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("hipMemcpy");
        sample.decodePacket(hc, dev_colour, rgba);
        sample.decodeDepthPacket(hd, dev_deep, depth);
        fovpt_warp_config wc;
        if (fovpt_warp_defaults(&wc) != FOVPT_OK) { printf("fovpt_warp_defaults failed\n"); return 2; }
        wc.images = FOVPT_WARP_RGBA;
        const fovpt_warp_camera to = sample.warpCamera(moved);
        sample.warpDepth(w, h, depth, hd.camera, to, wc, nullptr, rgba, nullptr, warped, map);
        struct fovpt_warp_counts counts = sample.warpCounts();
        if (counts.direct + counts.filled + counts.empty != n || counts.direct * 2 < n) { printf("the counts do not add up\n"); return 2; }
        std::vector<float> h_depth(n);
        std::vector<uint32_t> h_warped(n), h_map(n);
        if (hipMemcpy(h_depth.data(), depth, n * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(h_warped.data(), warped, n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(h_map.data(), map, n * 4, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("hipMemcpy");
        // the host decoder gives the device decoder's depths
        std::vector<float> host_depth(n, 0.0f);
        if (fovpt_packet_decode_depth_host(deep.data(), deep.size(), host_depth.data(), w, h) != FOVPT_OK || memcmp(host_depth.data(), h_depth.data(), n * 4) != 0) {
            printf("the host decoder's depths differ from the device decoder's\n");
            return 2;
        }
        // an output that is the depth image is an exception, like every other error of the shim
        if (!must_throw([&] { sample.warpDepth(w, h, depth, hd.camera, to, wc, nullptr, rgba, nullptr, warped, (uint32_t*)depth); }, "warpDepth into its depth image did not throw")) return 2;
        const uint32_t sizes[2] = {(uint32_t)colour.size(), (uint32_t)deep.size()};
        OutFile f(out);
        f.write(sizes, 4, 2);
        f.write(colour.data(), 1, colour.size());
        f.write(deep.data(), 1, deep.size());
        f.write(h_depth.data(), 4, n);
        f.write(h_warped.data(), 4, n);
        f.write(h_map.data(), 4, n);
        f.write(&counts, sizeof(counts), 1);
        f.close();
        for (void* p : {dev_colour, dev_deep, (void*)depth, (void*)rgba, (void*)warped, (void*)map}) (void)hipFree(p);
        printf("ok\n");
        return 0;
    });
}
