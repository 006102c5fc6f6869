// SimplePathtracer.h -- drop-in for PT_sv5_/SimplePathtracer.h: class SampleRenderer with the same
// public interface (ctor, render x2, resize, downloadPixels, setCamera, setProbe; public
// launchParams and stream), implemented over the C ABI of libfovpt (include/fovpt.h) instead of
// OptiX.  Header-only; link with -lfovpt.  Errors become std::runtime_error like the reference's
// sutil::Exception (sutil/Exception.h:245).
#pragma once
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

#include "LaunchParams.h"
#include "Model.h"
#include "sutil/Camera.h"

class SampleRenderer {
public:
    // performs all setup: device context + scene upload + LBVH build (SimplePathtracer.cpp:42-75)
    explicit SampleRenderer(const Model* model, int device = 0) : model(model)
    {
        if (fovpt_create(&ctx, device) != FOVPT_OK) throw std::runtime_error(fovpt_last_error(nullptr));
        std::vector<fovpt_mesh_desc> md(model->meshes.size());
        for (size_t i = 0; i < md.size(); i++) {
            const TriangleMesh& m = *model->meshes[i];
            md[i].vertex = m.vertex.empty() ? nullptr : &m.vertex[0].x;
            md[i].normal = m.normal.empty() ? nullptr : &m.normal[0].x;
            md[i].texcoord = m.texcoord.empty() ? nullptr : &m.texcoord[0].x;
            md[i].index = m.index.empty() ? nullptr : &m.index[0].x;
            md[i].num_vertices = (uint32_t)m.vertex.size();
            md[i].num_triangles = (uint32_t)m.index.size();
            md[i].texture_id = m.diffuseTextureID;
            static_assert(sizeof(Material) == sizeof(fovpt_material), "");
            md[i].material = *reinterpret_cast<const fovpt_material*>(&m.material);
        }
        std::vector<fovpt_texture_desc> td(model->textures.size());
        for (size_t i = 0; i < td.size(); i++) {
            td[i].pixel = model->textures[i]->pixel;
            td[i].width = model->textures[i]->resolution.x;
            td[i].height = model->textures[i]->resolution.y;
        }
        uint64_t trav = 0;
        check(fovpt_set_scene(ctx, md.data(), (int)md.size(), td.data(), (int)td.size(), &trav));
        launchParams.traversable = trav;
        stream = fovpt_stream(ctx);
    }
    ~SampleRenderer() { fovpt_destroy(ctx); }
    SampleRenderer(const SampleRenderer&) = delete;
    SampleRenderer& operator=(const SampleRenderer&) = delete;

    // one frame: the three foveation passes (or FOV_OFF), then a device sync (SimplePathtracer.cpp:77-214)
    void render()
    {
        check(fovpt_render(ctx, reinterpret_cast<fovpt_launch_params*>(&launchParams)));
        check(fovpt_synchronize(ctx));
    }
    // render into a caller-owned target: anything with `uint32_t* map()` / `void unmap()`, i.e. the shape
    // of sutil::CUDAOutputBuffer<uint32_t>.  Like the reference this repoints frame_buffer and leaves it (:218-219).
    template <typename Target>
    void render(Target& renderTarget)
    {
        uint32_t* result_buffer_data = renderTarget.map();
        launchParams.frame.frame_buffer = (uchar4*)result_buffer_data;
        render();
        renderTarget.unmap();
    }
    // the literal north-star overload: render with caller-held parameters
    void render(LaunchParams& params)
    {
        check(fovpt_render(ctx, reinterpret_cast<fovpt_launch_params*>(&params)));
        check(fovpt_synchronize(ctx));
    }
    void resize(const int2& newSize)
    {
        if (newSize.x == 0 || newSize.y == 0) return;
        fovpt_frame_ptrs p;
        check(fovpt_resize(ctx, newSize.x, newSize.y, &p));
        own_frame = p.frame_buffer;
        launchParams.frame.size = newSize;
        launchParams.frame.frame_buffer = (uchar4*)p.frame_buffer;
        launchParams.frame.accum_buffer = (float4*)p.accum_buffer;
        launchParams.frame.normal_buffer = (float4*)p.normal_buffer;
        launchParams.frame.color_buffer = (float4*)p.color_buffer;
        launchParams.frame.albedo_buffer = (float4*)p.albedo_buffer;
    }
    // always the renderer's own frame buffer (SimplePathtracer.cpp:276-280)
    void downloadPixels(uint32_t h_pixels[])
    {
        check(fovpt_download(ctx, own_frame, h_pixels, sizeof(uint32_t) * (size_t)launchParams.frame.size.x * (size_t)launchParams.frame.size.y));
    }
    void setCamera(const sutil::Camera& camera)
    {
        lastSetCamera = camera;
        lastSetCamera.setAspectRatio(launchParams.frame.size.x / float(launchParams.frame.size.y));
        lastSetCamera.UVWFrame(launchParams.camera.U, launchParams.camera.V, launchParams.camera.W);
        launchParams.camera.eye = lastSetCamera.eye();
    }
    void setProbe(const ProbeData& probe)
    {
        if (!probe.valid) throw std::runtime_error("Probe Data is not valid");       // Probe.h:104-105
        check(fovpt_set_probe(ctx, probe.width, probe.height, (const fovpt_float4*)probe.data, probe.pdfValuesX, probe.cdfValuesX,
                              probe.pdfValuesY, probe.cdfValuesY, (const fovpt_float3*)&probe.offset, &launchParams.probe));
    }
    // ---- denoiser (new with this library; replaces the reference family's OptiXDenoiser init / exec / finish and
    // computeFinalPixelColors, OtherProjects_01/06HelloPathtracing): filters the frame just rendered -- needs
    // fovpt_config.write_guides = 1 -- into the renderer's own buffers, then a device sync like render()
    void denoise() { fovpt_denoise_config dc; check(fovpt_denoise_defaults(&dc)); denoise(dc); }
    void denoise(const fovpt_denoise_config& dc)
    {
        check(fovpt_denoise(ctx, reinterpret_cast<const fovpt_launch_params*>(&launchParams), &dc, nullptr, nullptr));
        check(fovpt_synchronize(ctx));
    }
    // the denoised rgba8 pixels, like downloadPixels
    void downloadDenoisedPixels(uint32_t h_pixels[])
    {
        fovpt_float4* color = nullptr;
        uint32_t* rgba = nullptr;
        check(fovpt_denoise_buffers(ctx, &color, &rgba));
        check(fovpt_download(ctx, rgba, h_pixels, sizeof(uint32_t) * (size_t)launchParams.frame.size.x * (size_t)launchParams.frame.size.y));
    }
    // ---- reconstruction (new with this library; the reference family has none): rebuilds the block-filled middle ring and
    // periphery of the frame just rendered from a full-resolution G-buffer -- remodulate = 1 needs fovpt_config.write_guides = 1
    // -- into the renderer's own buffers, then a device sync like render().  in_color: nullptr = the accum buffer, or e.g. the
    // denoiser's colour output (fovpt_denoise_buffers)
    void reconstruct(const fovpt_float4* in_color = nullptr) { fovpt_reconstruct_config rc; check(fovpt_reconstruct_defaults(&rc)); reconstruct(rc, in_color); }
    void reconstruct(const fovpt_reconstruct_config& rc, const fovpt_float4* in_color = nullptr)
    {
        check(fovpt_reconstruct(ctx, reinterpret_cast<const fovpt_launch_params*>(&launchParams), &rc, in_color, nullptr, nullptr));
        check(fovpt_synchronize(ctx));
    }
    // the reconstructed rgba8 pixels, like downloadPixels
    void downloadReconstructedPixels(uint32_t h_pixels[])
    {
        fovpt_float4* color = nullptr;
        uint32_t* rgba = nullptr;
        check(fovpt_reconstruct_buffers(ctx, &color, &rgba));
        check(fovpt_download(ctx, rgba, h_pixels, sizeof(uint32_t) * (size_t)launchParams.frame.size.x * (size_t)launchParams.frame.size.y));
    }
    // ---- temporal reprojection (new with this library): one step of the renderer's frame history on the frame just rendered
    // (include/fovpt.h, fovpt_temporal) into the renderer's own buffers, then a device sync like render().  in_color: nullptr =
    // the accum buffer, or e.g. the reconstruction's colour output (fovpt_reconstruct_buffers)
    void temporal(const fovpt_float4* in_color = nullptr) { fovpt_temporal_config tc; check(fovpt_temporal_defaults(&tc)); temporal(tc, in_color); }
    void temporal(const fovpt_temporal_config& tc, const fovpt_float4* in_color = nullptr)
    {
        check(fovpt_temporal(ctx, reinterpret_cast<const fovpt_launch_params*>(&launchParams), &tc, in_color, nullptr, nullptr));
        check(fovpt_synchronize(ctx));
    }
    // drops the history (a caller that changes the lighting calls it: setProbe keeps the history)
    void temporal_reset() { check(fovpt_temporal_reset(ctx)); }
    // the temporal step's rgba8 pixels, like downloadPixels
    void downloadTemporalPixels(uint32_t h_pixels[])
    {
        fovpt_float4* color = nullptr;
        uint32_t* rgba = nullptr;
        const fovpt_float4* history = nullptr;
        check(fovpt_temporal_buffers(ctx, &color, &rgba, &history));
        check(fovpt_download(ctx, rgba, h_pixels, sizeof(uint32_t) * (size_t)launchParams.frame.size.x * (size_t)launchParams.frame.size.y));
    }
    // ---- the temporal step for animated scenes (include/fovpt.h, fovpt_temporal_motion): temporal() with the meshes updateAccel()
    // has moved since the previous step reprojected by their own motion -- the same history and buffers, so the two may be mixed.
    // out_motion: device memory for one float4 per pixel (px - x, py - y, depth in the previous camera, 1; zeros where the pixel
    // does not reproject), or nullptr.  Call it before updateAccel() moves the meshes for the next frame.
    void temporalMotion(const fovpt_float4* in_color = nullptr, fovpt_float4* out_motion = nullptr)
    {
        fovpt_temporal_config tc;
        check(fovpt_temporal_defaults(&tc));
        temporalMotion(tc, in_color, out_motion);
    }
    void temporalMotion(const fovpt_temporal_config& tc, const fovpt_float4* in_color = nullptr, fovpt_float4* out_motion = nullptr)
    {
        check(fovpt_temporal_motion(ctx, reinterpret_cast<const fovpt_launch_params*>(&launchParams), &tc, in_color, nullptr, nullptr, out_motion));
        check(fovpt_synchronize(ctx));
    }
    // the motion vectors a temporalMotion() wrote to d_motion, one float4 per pixel
    void downloadMotion(const fovpt_float4* d_motion, float4 h_motion[])
    {
        check(fovpt_download(ctx, d_motion, h_motion, sizeof(float4) * (size_t)launchParams.frame.size.x * (size_t)launchParams.frame.size.y));
    }
    // ---- the post-frame chain in one call (include/fovpt.h, fovpt_post): by default reconstruct() and temporalMotion() of the
    // frame just rendered, bit for bit, as one G-buffer trace and one kernel, into the renderer's own post buffers, then a device
    // sync like render().  pc.stages chooses the stages (FOVPT_POST_*); in_color and out_motion as in those calls
    void post()
    {
        fovpt_post_config pc;
        check(fovpt_post_defaults(&pc));
        post(pc);
    }
    void post(const fovpt_post_config& pc, const fovpt_float4* in_color = nullptr, fovpt_float4* out_motion = nullptr)
    {
        check(fovpt_post(ctx, reinterpret_cast<const fovpt_launch_params*>(&launchParams), &pc, in_color, nullptr, nullptr, out_motion));
        check(fovpt_synchronize(ctx));
    }
    // the chain's rgba8 pixels, like downloadPixels
    void downloadPostPixels(uint32_t h_pixels[])
    {
        fovpt_float4* color = nullptr;
        uint32_t* rgba = nullptr;
        check(fovpt_post_buffers(ctx, &color, &rgba));
        check(fovpt_download(ctx, rgba, h_pixels, sizeof(uint32_t) * (size_t)launchParams.frame.size.x * (size_t)launchParams.frame.size.y));
    }
    // ---- gaze-metered auto-exposure and tone map (include/fovpt.h, fovpt_expose): meters in_color (null: the accum buffer; by
    // default weighted by what the eye looks at), moves the renderer's exposure towards it and tone-maps the frame at that exposure
    // into the renderer's own exposed buffers, then a device sync like render().  Typically behind post(): exposePost()
    void expose()
    {
        fovpt_expose_config ec;
        check(fovpt_expose_defaults(&ec));
        expose(ec);
    }
    void expose(const fovpt_expose_config& ec, const fovpt_float4* in_color = nullptr)
    {
        check(fovpt_expose(ctx, reinterpret_cast<const fovpt_launch_params*>(&launchParams), &ec, in_color, nullptr, nullptr));
        check(fovpt_synchronize(ctx));
    }
    // expose() of the colour the last post() left in the renderer's own post buffers
    void exposePost(const fovpt_expose_config& ec)
    {
        fovpt_float4* color = nullptr;
        uint32_t* rgba = nullptr;
        check(fovpt_post_buffers(ctx, &color, &rgba));
        expose(ec, color);
    }
    struct fovpt_expose_state exposeState()
    {
        struct fovpt_expose_state s;
        check(fovpt_expose_state(ctx, &s));
        return s;
    }
    void exposeReset() { check(fovpt_expose_reset(ctx)); }
    // the exposed rgba8 pixels, like downloadPixels
    void downloadExposedPixels(uint32_t h_pixels[])
    {
        fovpt_float4* color = nullptr;
        uint32_t* rgba = nullptr;
        check(fovpt_expose_buffers(ctx, &color, &rgba));
        check(fovpt_download(ctx, rgba, h_pixels, sizeof(uint32_t) * (size_t)launchParams.frame.size.x * (size_t)launchParams.frame.size.y));
    }
    // ---- HDR glare ahead of the tone map (include/fovpt.h, fovpt_bloom): adds the glare of in_color's highlights (null: the accum
    // buffer) to it, into the renderer's own bloom buffers, then a device sync like render().  Meant ahead of expose(): exposeBloom()
    void bloom()
    {
        fovpt_bloom_config bc;
        check(fovpt_bloom_defaults(&bc));
        bloom(bc);
    }
    void bloom(const fovpt_bloom_config& bc, const fovpt_float4* in_color = nullptr)
    {
        check(fovpt_bloom(ctx, reinterpret_cast<const fovpt_launch_params*>(&launchParams), &bc, in_color, nullptr, nullptr));
        check(fovpt_synchronize(ctx));
    }
    // bloom() of the colour the last post() left in the renderer's own post buffers
    void bloomPost(const fovpt_bloom_config& bc)
    {
        fovpt_float4* color = nullptr;
        uint32_t* rgba = nullptr;
        check(fovpt_post_buffers(ctx, &color, &rgba));
        bloom(bc, color);
    }
    // expose() of the colour the last bloom() left in the renderer's own bloom buffers
    void exposeBloom(const fovpt_expose_config& ec)
    {
        fovpt_float4* color = nullptr;
        uint32_t* rgba = nullptr;
        check(fovpt_bloom_buffers(ctx, &color, &rgba));
        expose(ec, color);
    }
    // the bloom stage's float4 colour and rgba8 pixels, like downloadPixels
    void downloadBloomColor(fovpt_float4 h_color[])
    {
        fovpt_float4* color = nullptr;
        uint32_t* rgba = nullptr;
        check(fovpt_bloom_buffers(ctx, &color, &rgba));
        check(fovpt_download(ctx, color, h_color, sizeof(fovpt_float4) * (size_t)launchParams.frame.size.x * (size_t)launchParams.frame.size.y));
    }
    void downloadBloomPixels(uint32_t h_pixels[])
    {
        fovpt_float4* color = nullptr;
        uint32_t* rgba = nullptr;
        check(fovpt_bloom_buffers(ctx, &color, &rgba));
        check(fovpt_download(ctx, rgba, h_pixels, sizeof(uint32_t) * (size_t)launchParams.frame.size.x * (size_t)launchParams.frame.size.y));
    }
    // ---- late reprojection (include/fovpt.h, fovpt_warp): re-aims the frame just rendered at a newer camera -- its aspect ratio is
    // set from the frame size, as setCamera does -- into the renderer's own warped buffers, then a device sync like render().
    // in_color / in_rgba: null = the accum / frame buffer, or e.g. the exposed outputs (fovpt_expose_buffers).  reuse_gbuffer: take the
    // G-buffer of the last post() / temporal() step (fovpt_temporal_gbuffer) in place of tracing one
    void warp(const sutil::Camera& to, bool reuse_gbuffer = false, const fovpt_float4* in_color = nullptr, const uint32_t* in_rgba = nullptr)
    {
        fovpt_warp_config wc;
        check(fovpt_warp_defaults(&wc));
        warp(to, wc, reuse_gbuffer, in_color, in_rgba);
    }
    // `to` with the frame's aspect ratio, in the layout fovpt_warp, fovpt_warp_motion and fovpt_lens take
    fovpt_warp_camera warpCamera(const sutil::Camera& to) const
    {
        sutil::Camera cam = to;
        cam.setAspectRatio(launchParams.frame.size.x / float(launchParams.frame.size.y));
        float3 U, V, W;
        cam.UVWFrame(U, V, W);
        const float3 eye = cam.eye();
        fovpt_warp_camera wcam;
        wcam.eye.x = eye.x; wcam.eye.y = eye.y; wcam.eye.z = eye.z;
        wcam.U.x = U.x; wcam.U.y = U.y; wcam.U.z = U.z;
        wcam.V.x = V.x; wcam.V.y = V.y; wcam.V.z = V.z;
        wcam.W.x = W.x; wcam.W.y = W.y; wcam.W.z = W.z;
        return wcam;
    }
    void warp(const sutil::Camera& to, const fovpt_warp_config& wc, bool reuse_gbuffer = false, const fovpt_float4* in_color = nullptr,
              const uint32_t* in_rgba = nullptr)
    {
        const fovpt_warp_camera wcam = warpCamera(to);
        fovpt_gbuffer_ptrs g;
        if (reuse_gbuffer) check(fovpt_temporal_gbuffer(ctx, &g));
        check(fovpt_warp(ctx, reinterpret_cast<const fovpt_launch_params*>(&launchParams), &wcam, &wc, reuse_gbuffer ? &g : nullptr, in_color, in_rgba,
                         nullptr, nullptr, nullptr));
        check(fovpt_synchronize(ctx));
    }
    // ---- fovpt_warp_motion: warp() in which the meshes that moved in the interval the last post() / temporal step ended go on moving,
    // `advance` intervals past the rendered frame; into the same warped buffers, so downloadWarpedPixels and warpCounts serve both.
    // reuse_gbuffer: as warp()'s -- the hit records that go with the step's G-buffer are the context's last trace, which the library
    // checks to be of this frame
    void warpMotion(const sutil::Camera& to, float advance, bool reuse_gbuffer = false, const fovpt_float4* in_color = nullptr,
                    const uint32_t* in_rgba = nullptr)
    {
        fovpt_warp_motion_config mc;
        check(fovpt_warp_motion_defaults(&mc));
        mc.advance = advance;
        warpMotion(to, mc, reuse_gbuffer, in_color, in_rgba);
    }
    void warpMotion(const sutil::Camera& to, const fovpt_warp_motion_config& mc, bool reuse_gbuffer = false, const fovpt_float4* in_color = nullptr,
                    const uint32_t* in_rgba = nullptr)
    {
        const fovpt_warp_camera wcam = warpCamera(to);
        fovpt_gbuffer_ptrs g;
        if (reuse_gbuffer) check(fovpt_temporal_gbuffer(ctx, &g));
        check(fovpt_warp_motion(ctx, reinterpret_cast<const fovpt_launch_params*>(&launchParams), &wcam, &mc, reuse_gbuffer ? &g : nullptr, in_color,
                                in_rgba, nullptr, nullptr, nullptr));
        check(fovpt_synchronize(ctx));
    }
    // warpMotion() of the images the last expose() left in the renderer's own exposed buffers
    void warpMotionExposed(const sutil::Camera& to, float advance, bool reuse_gbuffer = false)
    {
        fovpt_float4* color = nullptr;
        uint32_t* rgba = nullptr;
        check(fovpt_expose_buffers(ctx, &color, &rgba));
        warpMotion(to, advance, reuse_gbuffer, color, rgba);
    }
    // warp() of the images the last expose() left in the renderer's own exposed buffers
    void warpExposed(const sutil::Camera& to, bool reuse_gbuffer = false)
    {
        fovpt_float4* color = nullptr;
        uint32_t* rgba = nullptr;
        check(fovpt_expose_buffers(ctx, &color, &rgba));
        warp(to, reuse_gbuffer, color, rgba);
    }
    struct fovpt_warp_counts warpCounts()
    {
        struct fovpt_warp_counts s;
        check(fovpt_warp_counts(ctx, &s));
        return s;
    }
    // the warped rgba8 pixels, like downloadPixels
    void downloadWarpedPixels(uint32_t h_pixels[])
    {
        fovpt_float4* color = nullptr;
        uint32_t* rgba = nullptr;
        check(fovpt_warp_buffers(ctx, &color, &rgba));
        check(fovpt_download(ctx, rgba, h_pixels, sizeof(uint32_t) * (size_t)launchParams.frame.size.x * (size_t)launchParams.frame.size.y));
    }
    // ---- gaze-metered focus distance and depth of field (include/fovpt.h, fovpt_focus): meters the distance of what the eye looks
    // at, moves the renderer's focus towards it and blurs in_color (null: the accum buffer) by a per-pixel radius around that
    // distance into the renderer's own focused buffers, then a device sync like render().  reuse_gbuffer: take the G-buffer of the
    // last post() / temporal() step (fovpt_temporal_gbuffer) in place of tracing one.  Typically behind post(): focusPost()
    void focus(bool reuse_gbuffer = false, const fovpt_float4* in_color = nullptr)
    {
        fovpt_focus_config fc;
        check(fovpt_focus_defaults(&fc));
        focus(fc, reuse_gbuffer, in_color);
    }
    void focus(const fovpt_focus_config& fc, bool reuse_gbuffer = false, const fovpt_float4* in_color = nullptr)
    {
        fovpt_gbuffer_ptrs g;
        if (reuse_gbuffer) check(fovpt_temporal_gbuffer(ctx, &g));
        check(fovpt_focus(ctx, reinterpret_cast<const fovpt_launch_params*>(&launchParams), &fc, reuse_gbuffer ? &g : nullptr, in_color, nullptr, nullptr,
                          nullptr));
        check(fovpt_synchronize(ctx));
    }
    // focus() of the colour the last post() left in the renderer's own post buffers, with that step's G-buffer
    void focusPost(const fovpt_focus_config& fc)
    {
        fovpt_float4* color = nullptr;
        uint32_t* rgba = nullptr;
        check(fovpt_post_buffers(ctx, &color, &rgba));
        focus(fc, true, color);
    }
    // cfg.strength of a thin lens of radius lens_radius (scene units) at the current camera and frame height
    float focusStrength(float lens_radius) const
    {
        const float3 V = launchParams.camera.V, W = launchParams.camera.W;
        return lens_radius * (launchParams.frame.size.y * 0.5f) * sqrtf(W.x * W.x + W.y * W.y + W.z * W.z) / sqrtf(V.x * V.x + V.y * V.y + V.z * V.z);
    }
    struct fovpt_focus_state focusState()
    {
        struct fovpt_focus_state s;
        check(fovpt_focus_state(ctx, &s));
        return s;
    }
    void focusReset() { check(fovpt_focus_reset(ctx)); }
    // the focused float4 colour (may be null) and rgba8 pixels (may be null), like downloadPixels
    void downloadFocus(fovpt_float4 h_color[], uint32_t h_pixels[])
    {
        fovpt_float4* color = nullptr;
        uint32_t* rgba = nullptr;
        check(fovpt_focus_buffers(ctx, &color, &rgba));
        const size_t n = (size_t)launchParams.frame.size.x * (size_t)launchParams.frame.size.y;
        if (h_color) check(fovpt_download(ctx, color, h_color, sizeof(fovpt_float4) * n));
        if (h_pixels) check(fovpt_download(ctx, rgba, h_pixels, sizeof(uint32_t) * n));
    }
    // ---- head-mounted display lens pre-distortion with chromatic correction (include/fovpt.h, fovpt_lens): resamples in_color (null:
    // the accum buffer; typically expose()'s colour) through the lens polynomial, one position per colour channel, into the
    // renderer's own lens buffers, then a device sync like render().  `to` (may be null): a late camera whose ROTATION re-aims the
    // rays in the same gather.  lens() without a configuration: lensForFrame(lensDefaults())
    static fovpt_lens_config lensDefaults()
    {
        fovpt_lens_config lc;
        if (fovpt_lens_defaults(&lc) != FOVPT_OK) throw std::runtime_error("fovpt_lens_defaults failed");
        return lc;
    }
    // lc fitted to the renderer's frame size: scale.y = h / w, src_scale.y = w / h, both src_scale entries divided by f(1), so that
    // the mid-point of the left and right edges maps to itself
    fovpt_lens_config lensForFrame(const fovpt_lens_config& lc) const
    {
        fovpt_lens_config c = lc;
        const double w = launchParams.frame.size.x, h = launchParams.frame.size.y;
        const double f1 = (double)c.k[0] + ((double)c.k[1] + ((double)c.k[2] + (double)c.k[3]));
        c.scale[1] = (float)(h / w);
        c.src_scale[1] = (float)(w / h);
        c.src_scale[0] = (float)((double)c.src_scale[0] / f1);
        c.src_scale[1] = (float)((double)c.src_scale[1] / f1);
        return c;
    }
    void lens(const sutil::Camera* to = nullptr, const fovpt_float4* in_color = nullptr) { lens(lensForFrame(lensDefaults()), to, in_color); }
    void lens(const fovpt_lens_config& lc, const sutil::Camera* to = nullptr, const fovpt_float4* in_color = nullptr)
    {
        fovpt_warp_camera wcam;
        if (to) wcam = warpCamera(*to);
        check(fovpt_lens(ctx, reinterpret_cast<const fovpt_launch_params*>(&launchParams), &lc, to ? &wcam : nullptr, in_color, nullptr, nullptr));
        check(fovpt_synchronize(ctx));
    }
    void lensBuffers(fovpt_float4** color, uint32_t** rgba) { check(fovpt_lens_buffers(ctx, color, rgba)); }
    // the pre-distorted float4 colour (may be null) and rgba8 pixels (may be null), like downloadPixels
    void downloadLens(fovpt_float4 h_color[], uint32_t h_pixels[])
    {
        fovpt_float4* color = nullptr;
        uint32_t* rgba = nullptr;
        check(fovpt_lens_buffers(ctx, &color, &rgba));
        const size_t n = (size_t)launchParams.frame.size.x * (size_t)launchParams.frame.size.y;
        if (h_color) check(fovpt_download(ctx, color, h_color, sizeof(fovpt_float4) * n));
        if (h_pixels) check(fovpt_download(ctx, rgba, h_pixels, sizeof(uint32_t) * n));
    }
    // ---- luminance moment history and variance-guided a-trous filter (include/fovpt.h, fovpt_variance / fovpt_variance_filter).
    // variance(): one step of the moment history of the frame last rendered into the renderer's own variance image (or
    // out_variance); gbuffer null: traced by the call; in_sample null: the accum buffer; motion (may be null): the motion vectors
    // post() / temporalMotion() write.  varianceFilter(): filters in_color (null: the accum buffer; typically post()'s colour) by
    // `variance` (null: the renderer's own image) into the renderer's own buffers (or the caller's).  Both are only enqueued;
    // downloadVarianceFiltered() synchronises
    static fovpt_variance_config varianceDefaults()
    {
        fovpt_variance_config vc;
        if (fovpt_variance_defaults(&vc) != FOVPT_OK) throw std::runtime_error("fovpt_variance_defaults failed");
        return vc;
    }
    void variance() { variance(varianceDefaults()); }
    void variance(const fovpt_variance_config& vc, const fovpt_gbuffer_ptrs* gbuffer = nullptr, const fovpt_float4* in_sample = nullptr,
                  const fovpt_float4* motion = nullptr, fovpt_float4* out_variance = nullptr)
    {
        check(fovpt_variance(ctx, reinterpret_cast<const fovpt_launch_params*>(&launchParams), &vc, gbuffer, in_sample, motion, out_variance));
    }
    void varianceBuffers(fovpt_float4** variance, const fovpt_float4** moments) { check(fovpt_variance_buffers(ctx, variance, moments)); }
    void varianceReset() { check(fovpt_variance_reset(ctx)); }
    // the renderer's own variance image, (rel, var, mean, n) per pixel
    void downloadVariance(fovpt_float4 h_variance[])
    {
        fovpt_float4* var = nullptr;
        const fovpt_float4* moments = nullptr;
        check(fovpt_variance_buffers(ctx, &var, &moments));
        check(fovpt_download(ctx, var, h_variance, sizeof(fovpt_float4) * (size_t)launchParams.frame.size.x * (size_t)launchParams.frame.size.y));
    }
    static fovpt_variance_filter_config varianceFilterDefaults()
    {
        fovpt_variance_filter_config fc;
        if (fovpt_variance_filter_defaults(&fc) != FOVPT_OK) throw std::runtime_error("fovpt_variance_filter_defaults failed");
        return fc;
    }
    void varianceFilter() { varianceFilter(varianceFilterDefaults()); }
    void varianceFilter(const fovpt_variance_filter_config& fc, const fovpt_gbuffer_ptrs* gbuffer = nullptr, const fovpt_float4* in_color = nullptr,
                        const fovpt_float4* variance = nullptr, fovpt_float4* out_color = nullptr, uint32_t* out_rgba = nullptr)
    {
        check(fovpt_variance_filter(ctx, reinterpret_cast<const fovpt_launch_params*>(&launchParams), &fc, gbuffer, in_color, variance, out_color, out_rgba));
    }
    void varianceFilterBuffers(fovpt_float4** color, uint32_t** rgba) { check(fovpt_variance_filter_buffers(ctx, color, rgba)); }
    // behind post(pc, nullptr, motion): a moment step on the raw samples (the accum buffer) and the filter of the colour post() left
    // in the renderer's own post buffers, both with that step's G-buffer (no trace of their own); motion: what post() wrote, or null
    void variancePost(const fovpt_variance_config& vc, const fovpt_variance_filter_config& fc, const fovpt_float4* motion = nullptr)
    {
        fovpt_gbuffer_ptrs g;
        check(fovpt_temporal_gbuffer(ctx, &g));
        fovpt_float4* color = nullptr;
        uint32_t* rgba = nullptr;
        check(fovpt_post_buffers(ctx, &color, &rgba));
        variance(vc, &g, nullptr, motion);
        varianceFilter(fc, &g, color);
    }
    // the filtered rgba8 pixels (may be null) and float4 colour (may be null), like downloadPixels
    void downloadVarianceFiltered(uint32_t h_pixels[], fovpt_float4 h_color[] = nullptr)
    {
        fovpt_float4* color = nullptr;
        uint32_t* rgba = nullptr;
        check(fovpt_variance_filter_buffers(ctx, &color, &rgba));
        const size_t n = (size_t)launchParams.frame.size.x * (size_t)launchParams.frame.size.y;
        if (h_color) check(fovpt_download(ctx, color, h_color, sizeof(fovpt_float4) * n));
        if (h_pixels) check(fovpt_download(ctx, rgba, h_pixels, sizeof(uint32_t) * n));
    }
    // ---- image quality of the frame last rendered (include/fovpt.h, fovpt_quality): test_rgba (null: the frame buffer) against
    // ref_rgba, device rgba8 images of the frame's size -> per-class error sums, SSIM sums and the eccentricity profile; the scores
    // of a record are fovpt_quality_mse / _psnr / _ssim / _score.  measureQuality() measures into the renderer's own record and
    // reads it (a device sync); qualityAsync() only enqueues (out_sums: a device record of the caller's, null: the renderer's own,
    // which readQuality() returns); out_class (device, may be null): one byte per pixel, its class
    static fovpt_quality_config qualityDefaults()
    {
        fovpt_quality_config qc;
        if (fovpt_quality_defaults(&qc) != FOVPT_OK) throw std::runtime_error("fovpt_quality_defaults failed");
        return qc;
    }
    void qualityAsync(const uint32_t* ref_rgba, const uint32_t* test_rgba = nullptr, const fovpt_quality_config* qc = nullptr,
                      fovpt_quality_sums* out_sums = nullptr, uint8_t* out_class = nullptr)
    {
        const fovpt_quality_config d = qc ? *qc : qualityDefaults();
        check(fovpt_quality(ctx, reinterpret_cast<const fovpt_launch_params*>(&launchParams), &d, test_rgba, ref_rgba, out_sums, out_class));
    }
    fovpt_quality_sums readQuality()
    {
        fovpt_quality_sums s;
        check(fovpt_quality_read(ctx, &s));
        return s;
    }
    fovpt_quality_sums measureQuality(const uint32_t* ref_rgba, const uint32_t* test_rgba = nullptr, const fovpt_quality_config* qc = nullptr,
                                      uint8_t* out_class = nullptr)
    {
        qualityAsync(ref_rgba, test_rgba, qc, nullptr, out_class);
        return readQuality();
    }
    // ---- foveated frame packets (include/fovpt.h, fovpt_packet_*): the frame last rendered -- in_rgba null: the renderer's own
    // frame buffer; or the rgba8 output of post() / expose() -- as a small self-describing packet in pinned host memory, without a
    // device sync: submitPacket() returns at once with a slot, later frames keep rendering, waitPacket(slot) waits for that
    // slot's copy alone.  A client decodes the bytes with fovpt_packet_decode_host (libfovpt_loader.so has it: no ROCm needed)
    struct Packet { const void* data; size_t bytes; };
    int submitPacket(uint32_t sequence, const uint32_t* in_rgba = nullptr)
    {
        int slot = -1;
        check(fovpt_packet_submit(ctx, reinterpret_cast<const fovpt_launch_params*>(&launchParams), in_rgba, sequence, &slot));
        return slot;
    }
    // the same as a coded packet ("FVPC"): codec.codec[p] says whether launch pass p goes as raw texels or as BC1 blocks
    // (fovpt_packet_defaults: BC1 where the pass's fill is above 1, so the fovea stays exact); the slots are the same
    int submitPacket(uint32_t sequence, const fovpt_packet_config& codec, const uint32_t* in_rgba = nullptr)
    {
        int slot = -1;
        check(fovpt_packet_submit_coded(ctx, reinterpret_cast<const fovpt_launch_params*>(&launchParams), &codec, in_rgba, sequence, &slot));
        return slot;
    }
    // valid until the slot is submitted again (FOVPT_PACKET_SLOTS submits later)
    Packet waitPacket(int slot)
    {
        Packet p = {nullptr, 0};
        check(fovpt_packet_wait(ctx, slot, &p.data, &p.bytes));
        return p;
    }
    // the device decoder: header on the host, packet and out_rgba (the header's width x height pixels) on the device; enqueued on
    // the renderer's stream, then a device sync like render()
    void decodePacket(const fovpt_packet_header& header, const void* packet, uint32_t* out_rgba, int mode = FOVPT_PACKET_NEAREST)
    {
        check(fovpt_packet_decode(ctx, &header, packet, mode, out_rgba));
        check(fovpt_synchronize(ctx));
    }
    // ---- depth packets and the client's warp (include/fovpt.h, "depth packets"): the frame's depth and camera travel like its
    // colour -- submitDepthPacket() beside submitPacket(), the same slots and waitPacket() --, and a client that holds no scene
    // decodes both and re-aims the image itself: decodePacket, decodeDepthPacket, warpDepth.  reuse_gbuffer: as warp()'s
    int submitDepthPacket(uint32_t sequence, bool reuse_gbuffer = false, float near = 0.1f)
    {
        fovpt_packet_depth_config cfg;
        fovpt_packet_depth_defaults(&cfg);
        cfg.near = near;
        fovpt_gbuffer_ptrs g;
        if (reuse_gbuffer) check(fovpt_temporal_gbuffer(ctx, &g));
        int slot = -1;
        check(fovpt_packet_submit_depth(ctx, reinterpret_cast<const fovpt_launch_params*>(&launchParams), &cfg, reuse_gbuffer ? &g : nullptr, sequence, &slot));
        return slot;
    }
    // the device decoder: header on the host, packet and out_depth (the header's width x height floats, +inf the sky) on the
    // device; needs no scene and no rendered frame; then a device sync like render()
    void decodeDepthPacket(const fovpt_packet_depth_header& header, const void* packet, float* out_depth)
    {
        check(fovpt_packet_decode_depth(ctx, &header, packet, out_depth));
        check(fovpt_synchronize(ctx));
    }
    // fovpt_warp from a decoded depth image and the camera in the depth packet's header to the camera `to`; every buffer is the
    // caller's, on the device (in_color / out_color may be null where wc leaves the float4 image out); warpCounts() reports it
    void warpDepth(int width, int height, const float* depth, const fovpt_warp_camera& from, const fovpt_warp_camera& to, const fovpt_warp_config& wc,
                   const fovpt_float4* in_color, const uint32_t* in_rgba, fovpt_float4* out_color, uint32_t* out_rgba, uint32_t* out_map = nullptr)
    {
        check(fovpt_warp_depth(ctx, width, height, &from, &to, &wc, depth, in_color, in_rgba, out_color, out_rgba, out_map));
        check(fovpt_synchronize(ctx));
    }
    // ---- animated geometry (new with this library; OptiX's optixAccelBuild with OPERATION_UPDATE over the same build inputs):
    // re-reads model->meshes[i]->vertex of the listed meshes from the Model this renderer was built over and refits the
    // hierarchy on the library's stream (asynchronous: frames rendered afterwards see the new positions), or with rebuild = true
    // builds it anew (synchronous; include/fovpt.h, fovpt_update_vertices).  `rebuild` of the whole updateAccel family has a third
    // choice, REBUILD_ASYNC: the call refits, and a new hierarchy is built beside the frames and adopted by a later update or by
    // rebuildState(false, true) (include/fovpt.h, FOVPT_UPDATE_REBUILD_ASYNC)
    enum { REFIT = 0, REBUILD = 1, REBUILD_ASYNC = 2 };        // (false and true still mean the first two)
    static constexpr int rebuildFlag(int rebuild) { return rebuild == REBUILD_ASYNC ? FOVPT_UPDATE_REBUILD_ASYNC : rebuild ? FOVPT_UPDATE_REBUILD : 0; }
    // the background rebuild's state and counters; wait: until it is not BUILDING (never for the device); adopt: now, if READY
    fovpt_rebuild_info rebuildState(bool wait = false, bool adopt = false)
    {
        fovpt_rebuild_info info;
        check(fovpt_rebuild_state(ctx, (wait ? FOVPT_REBUILD_WAIT : 0) | (adopt ? FOVPT_REBUILD_ADOPT : 0), &info));
        return info;
    }
    void updateAccel(const std::vector<int>& meshes, int rebuild = REFIT)
    {
        std::vector<fovpt_vertex_update> up(meshes.size());
        for (size_t k = 0; k < meshes.size(); k++) {
            if (meshes[k] < 0 || (size_t)meshes[k] >= model->meshes.size()) throw std::runtime_error("updateAccel: mesh index out of range");
            const TriangleMesh& m = *model->meshes[meshes[k]];
            up[k].mesh = meshes[k];
            up[k].num_vertices = (uint32_t)m.vertex.size();
            up[k].vertex = m.vertex.empty() ? nullptr : &m.vertex[0].x;
        }
        check(fovpt_update_vertices(ctx, up.data(), (int)up.size(), rebuildFlag(rebuild)));
    }
    // rigid motion: the listed meshes' rest positions (the Model's, when this renderer was built) through row-major 3 x 4
    // matrices on the device, absolute not cumulative, then updateAccel()'s refit or rebuild (include/fovpt.h,
    // fovpt_update_transforms).  The Model is not changed.
    void updateTransforms(const std::vector<fovpt_mesh_transform>& transforms, int rebuild = REFIT)
    {
        check(fovpt_update_transforms(ctx, transforms.data(), (int)transforms.size(), rebuildFlag(rebuild)));
    }
    // the SAH cost of the hierarchy as built and as last measured (include/fovpt.h, fovpt_hierarchy_cost): the first call
    // switches the measurements on; wait = false never blocks and may lag, wait = true returns measured == updates.  Rebuild
    // when current / built passes your threshold.
    fovpt_hierarchy_cost_info hierarchyCost(bool wait = false)
    {
        fovpt_hierarchy_cost_info info;
        check(fovpt_hierarchy_cost(ctx, wait ? FOVPT_COST_WAIT : 0, &info));
        return info;
    }
    // skinning: setSkins uploads, replaces or removes (num_joints 0, null pointers) the skins of the listed meshes, once;
    // updateSkinned sends their palettes (num_joints row-major 3 x 4 matrices each; device = true: device pointers, read in
    // stream order) and blends them per vertex over the rest positions on the device, absolute not cumulative, then
    // updateAccel()'s refit or rebuild (include/fovpt.h, fovpt_set_skins / fovpt_update_skinned).  The Model is not changed.
    fovpt_ctx* context() const { return ctx; }       // the C ABI's context, for calls this class does not wrap (fovpt_debug_buffer)
    void setSkins(const std::vector<fovpt_mesh_skin>& skins) { check(fovpt_set_skins(ctx, skins.data(), (int)skins.size())); }
    void updateSkinned(const std::vector<fovpt_skin_pose>& poses, int rebuild = REFIT, bool device = false)
    {
        check(fovpt_update_skinned(ctx, poses.data(), (int)poses.size(), rebuildFlag(rebuild) | (device ? FOVPT_UPDATE_DEVICE : 0)));
    }
    // morph targets: setMorphs uploads, replaces or removes (num_targets 0, null pointer) the targets of the listed meshes,
    // once; updateMorphed sends one weight per target and, with num_joints > 0, the mesh's skin palette (device = true: device
    // pointers, read in stream order), adds the weighted deltas to the rest positions on the device and sends the result
    // through the skin, absolute not cumulative, then updateAccel()'s refit or rebuild (include/fovpt.h, fovpt_set_morphs /
    // fovpt_update_morphed).  The Model is not changed.
    void setMorphs(const std::vector<fovpt_mesh_morph>& morphs) { check(fovpt_set_morphs(ctx, morphs.data(), (int)morphs.size())); }
    void updateMorphed(const std::vector<fovpt_morph_pose>& poses, int rebuild = REFIT, bool device = false)
    {
        check(fovpt_update_morphed(ctx, poses.data(), (int)poses.size(), rebuildFlag(rebuild) | (device ? FOVPT_UPDATE_DEVICE : 0)));
    }
    // rigs: setRig uploads the node hierarchy, the bindings of meshes to it and the keyframe clips, once (after setSkins /
    // setMorphs, either of which drops the rig; nullptr removes it); updateAnimated samples clip `clip` at `time`, composes the
    // hierarchy and poses every bound mesh on the device, absolute not cumulative, then updateAccel()'s refit or rebuild
    // (include/fovpt.h, fovpt_set_rig / fovpt_update_animated).  The caller wraps its own time to loop.  The Model is not changed.
    void setRig(const fovpt_rig_desc* rig) { check(fovpt_set_rig(ctx, rig)); }
    void updateAnimated(int clip, float time, int rebuild = REFIT) { check(fovpt_update_animated(ctx, clip, time, rebuildFlag(rebuild))); }
    // ---- multi-GPU (new with this library; the reference is single-GPU): one SampleRenderer per GPU / process, rank and
    // world in fovpt_config, the framebuffer gathered over RCCL on the library's stream (include/fovpt.h, fovpt_comm_*)
    void renderAsync() { check(fovpt_render(ctx, reinterpret_cast<fovpt_launch_params*>(&launchParams))); }   // render() without the sync
    // frames issued with renderAsync() run up to two at a time (fovpt_config.frames_in_flight: 2 = throughput, the default;
    // 1 = lowest latency per frame); they complete in order on `stream`
    void setFramesInFlight(int n) { fovpt_config c = config(); c.frames_in_flight = n; setConfig(c); }
    void commInit(const void* uniqueId, int rank, int world) { check(fovpt_comm_init(ctx, uniqueId, rank, world)); }
    // gathers the frame just rendered (the renderer's current frame_buffer) onto `root`; fullFrame: device memory, root only
    void gatherFrame(int root, uint32_t* fullFrame)
    {
        check(fovpt_gather_frame(ctx, reinterpret_cast<const fovpt_launch_params*>(&launchParams), root,
                                 (const uint32_t*)launchParams.frame.frame_buffer, fullFrame));
    }
    // the reference's compile-time switches (FOV_ON/OFF, radii, spp, depth) as run-time settings
    fovpt_config config() const { fovpt_config c; fovpt_get_config(ctx, &c); return c; }
    void setConfig(const fovpt_config& c) { check(fovpt_set_config(ctx, &c)); }

    LaunchParams launchParams;       // public and caller-mutated, as in the reference (SimplePathtracer.h:146)
    void* stream = nullptr;          // hipStream_t
    sutil::Camera lastSetCamera;
    const Model* model;

private:
    void check(int rc) const
    {
        if (rc != FOVPT_OK) throw std::runtime_error(std::string("libfovpt: ") + fovpt_last_error(ctx));
    }
    fovpt_ctx* ctx = nullptr;
    uint32_t* own_frame = nullptr;
};
