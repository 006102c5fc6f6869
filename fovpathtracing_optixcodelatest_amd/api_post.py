"""The post-frame stages of SampleRenderer, beside csrc/api_post.hip: denoise, G-buffer, reconstruct, temporal, post, expose, bloom,
warp, focus, lens, variance and quality.  A stage is one block: its defaults, the call, its own buffers and their downloads."""
import ctypes as C
import math

import numpy as np

from . import abi, lib


def _defaults(name, cls):
    """A cls() filled by fovpt_<name>_defaults."""
    d = cls()
    lib.check(None, getattr(lib.load(), "fovpt_%s_defaults" % name)(C.byref(d)))
    return d


def _ref(x):
    """byref(x), or None (a null pointer) for None."""
    return C.byref(x) if x is not None else None


class PostStages:
    """Mixed into SampleRenderer (renderer.py), which brings _L, _ctx, _check, launchParams, download and _download_frame."""

    def _own_buffers(self, name, n=2):
        """The n device addresses fovpt_<name>_buffers gives: the renderer's own outputs of that stage, as a tuple."""
        ptrs = [C.c_void_p() for _ in range(n)]
        self._check(getattr(self._L, "fovpt_%s_buffers" % name)(self._ctx, *[C.byref(p) for p in ptrs]))
        return tuple(p.value for p in ptrs)

    def _device_tensor(self, make):
        """make(torch, device string): a torch tensor on this renderer's device, complete before this returns."""
        import torch
        t = make(torch, "cuda:%d" % self._device)
        torch.cuda.synchronize(self._device)
        return t

    # -- denoiser of the rendered frame (include/fovpt.h, fovpt_denoise): in place of the reference family's OptiXDenoiser
    @staticmethod
    def denoise_defaults() -> abi.DenoiseConfig:
        return _defaults("denoise", abi.DenoiseConfig)

    def denoise(self, cfg=None, out_color=None, out_rgba=None):
        """Filters the frame last rendered (needs config.write_guides = 1).  out_color / out_rgba: device pointers (float4 /
        rgba8 per pixel), or None for the renderer's own buffers (downloadDenoisedColor / downloadDenoisedPixels).  Enqueued on
        the renderer's stream, not synchronised (the downloads synchronise)."""
        cfg = cfg if cfg is not None else self.denoise_defaults()
        self._check(self._L.fovpt_denoise(self._ctx, C.byref(self.launchParams), C.byref(cfg), out_color, out_rgba))

    def denoise_buffers(self):
        """Device addresses of the renderer's own denoiser outputs: (float4 colour, rgba8)."""
        return self._own_buffers("denoise")

    def downloadDenoisedPixels(self):
        """The rgba8 output of the last denoise into the renderer's own buffer, shaped like downloadPixels()."""
        return self._download_frame(self._own_buffers("denoise")[1], 1)

    def downloadDenoisedColor(self):
        """The float4 output of the last denoise into the renderer's own buffer."""
        return self._download_frame(self._own_buffers("denoise")[0], 4)

    # -- G-buffer and reconstruction of the rendered frame (include/fovpt.h, fovpt_gbuffer / fovpt_reconstruct)
    def gbuffer(self) -> abi.GBufferPtrs:
        """Enqueues the primary-visibility G-buffer of the current frame size and camera on the renderer's stream (not
        synchronised) and returns its device pointers (prim uint32, position / normal / albedo float4 per pixel)."""
        g = abi.GBufferPtrs()
        self._check(self._L.fovpt_gbuffer(self._ctx, C.byref(self.launchParams), C.byref(g)))
        return g

    def downloadGBuffer(self, g=None):
        """The G-buffer as numpy arrays {prim (H, W) uint32, position / normal / albedo (H, W, 4) float32}; g: what gbuffer()
        returned (None: build it now)."""
        g = g if g is not None else self.gbuffer()
        shape = (g.height, g.width)
        out = dict(prim=self.download(g.prim, np.empty(shape, np.uint32)))
        for k in ("position", "normal", "albedo"):
            out[k] = self.download(getattr(g, k), np.empty(shape + (4,), np.float32))
        return out

    @staticmethod
    def reconstruct_defaults() -> abi.ReconstructConfig:
        return _defaults("reconstruct", abi.ReconstructConfig)

    def reconstruct(self, cfg=None, in_color=None, out_color=None, out_rgba=None):
        """Reconstructs the block-filled pixels of the frame last rendered (remodulate = 1 needs config.write_guides = 1).
        in_color: device pointer of a float4 frame (None: the accum buffer; e.g. denoise_buffers()[0]).  out_color / out_rgba:
        device pointers, or None for the renderer's own buffers (downloadReconstructedColor / downloadReconstructedPixels).
        Enqueued on the renderer's stream, not synchronised (the downloads synchronise)."""
        cfg = cfg if cfg is not None else self.reconstruct_defaults()
        self._check(self._L.fovpt_reconstruct(self._ctx, C.byref(self.launchParams), C.byref(cfg), in_color, out_color, out_rgba))

    def reconstruct_buffers(self):
        """Device addresses of the renderer's own reconstruction outputs: (float4 colour, rgba8)."""
        return self._own_buffers("reconstruct")

    def downloadReconstructedPixels(self):
        """The rgba8 output of the last reconstruct into the renderer's own buffer, shaped like downloadPixels()."""
        return self._download_frame(self._own_buffers("reconstruct")[1], 1)

    def downloadReconstructedColor(self):
        """The float4 output of the last reconstruct into the renderer's own buffer."""
        return self._download_frame(self._own_buffers("reconstruct")[0], 4)

    # -- temporal reprojection of the frame history (include/fovpt.h, fovpt_temporal)
    @staticmethod
    def temporal_defaults() -> abi.TemporalConfig:
        return _defaults("temporal", abi.TemporalConfig)

    def temporal(self, cfg=None, in_color=None, out_color=None, out_rgba=None):
        """One step of the renderer's frame history on the frame last rendered.  in_color: device pointer of a float4 frame
        (None: the accum buffer; e.g. reconstruct_buffers()[0]).  out_color / out_rgba: device pointers (out_color may be
        in_color), or None for the renderer's own buffers (downloadTemporalColor / downloadTemporalPixels).  Enqueued on the
        renderer's stream, not synchronised (the downloads synchronise)."""
        cfg = cfg if cfg is not None else self.temporal_defaults()
        self._check(self._L.fovpt_temporal(self._ctx, C.byref(self.launchParams), C.byref(cfg), in_color, out_color, out_rgba))

    def temporal_buffers(self):
        """Device addresses of the renderer's own temporal outputs and of the history the last step wrote: (float4 colour,
        rgba8, float4 history (rgb, history length))."""
        return self._own_buffers("temporal", 3)

    def temporal_reset(self):
        """Drops the frame history: the next temporal() step outputs its input."""
        self._check(self._L.fovpt_temporal_reset(self._ctx))

    def downloadTemporalPixels(self):
        """The rgba8 output of the last temporal step into the renderer's own buffer, shaped like downloadPixels()."""
        return self._download_frame(self._own_buffers("temporal", 3)[1], 1)

    def downloadTemporalColor(self):
        """The float4 output of the last temporal step into the renderer's own buffer."""
        return self._download_frame(self._own_buffers("temporal", 3)[0], 4)

    def downloadTemporalHistory(self):
        """The history the last temporal step wrote: (H, W, 4) float32, rgb its output colour, w the history length."""
        return self._download_frame(self._own_buffers("temporal", 3)[2], 4)

    # -- the temporal step for animated scenes (include/fovpt.h, fovpt_temporal_motion)
    def temporal_motion(self, cfg=None, in_color=None, out_color=None, out_rgba=None, out_motion=None):
        """temporal() with the meshes update_vertices() has moved since the previous step reprojected by their own motion: the
        same history, buffers and ordering.  out_motion: device pointer of a float4 frame for the per-pixel motion vectors
        (px - x, py - y, depth in the previous camera, 1), zeros where the pixel does not reproject; None: none are written
        (motion_buffer() is the renderer's own).  Call it before update_vertices() moves the meshes for the next frame."""
        cfg = cfg if cfg is not None else self.temporal_defaults()
        self._check(self._L.fovpt_temporal_motion(self._ctx, C.byref(self.launchParams), C.byref(cfg), in_color, out_color, out_rgba,
                                                  out_motion))

    def motion_buffer(self):
        """Device address of the renderer's own motion-vector buffer (float4 per pixel of the current frame size), made on
        first use and after a resize: pass it as temporal_motion(out_motion=...), read it with downloadMotion()."""
        f = self.launchParams.frame
        shape = (f.size.y, f.size.x, 4)
        if self._motion is None or tuple(self._motion.shape) != shape:
            self.synchronize()                 # (a step may still be writing the buffer this one replaces)
            self._motion = self._device_tensor(lambda torch, dev: torch.zeros(shape, dtype=torch.float32, device=dev))
        return self._motion.data_ptr()

    def downloadMotion(self):
        """The motion vectors the last temporal_motion(out_motion=motion_buffer()) wrote: (H, W, 4) float32."""
        return self._download_frame(self.motion_buffer(), 4)

    # -- the post-frame chain in one call (include/fovpt.h, fovpt_post)
    @staticmethod
    def post_defaults() -> abi.PostConfig:
        return _defaults("post", abi.PostConfig)

    def post(self, cfg=None, in_color=None, out_color=None, out_rgba=None, out_motion=None):
        """The stages of cfg.stages (abi.POST_DENOISE | POST_RECONSTRUCT | POST_TEMPORAL | POST_MOTION; default reconstruct,
        temporal, motion) on the frame last rendered, bit for bit denoise(), reconstruct() and temporal() / temporal_motion() made
        one after the other -- with reconstruct and temporal both on as one G-buffer trace and one kernel.  in_color: device
        pointer of a float4 frame (None: the accum buffer; not with POST_DENOISE).  out_color / out_rgba: device pointers, or None
        for the renderer's own buffers (downloadPostColor / downloadPostPixels); out_motion as temporal_motion()'s.  Enqueued
        on the renderer's stream, not synchronised (the downloads synchronise)."""
        cfg = cfg if cfg is not None else self.post_defaults()
        self._check(self._L.fovpt_post(self._ctx, C.byref(self.launchParams), C.byref(cfg), in_color, out_color, out_rgba, out_motion))

    def post_buffers(self):
        """Device addresses of the renderer's own post outputs: (float4 colour, rgba8)."""
        return self._own_buffers("post")

    def downloadPostPixels(self):
        """The rgba8 output of the last post() into the renderer's own buffer, shaped like downloadPixels()."""
        return self._download_frame(self._own_buffers("post")[1], 1)

    def downloadPostColor(self):
        """The float4 output of the last post() into the renderer's own buffer."""
        return self._download_frame(self._own_buffers("post")[0], 4)

    # -- gaze-metered auto-exposure and tone map (include/fovpt.h, fovpt_expose)
    @staticmethod
    def expose_defaults() -> abi.ExposeConfig:
        return _defaults("expose", abi.ExposeConfig)

    def expose(self, cfg=None, in_color=None, out_color=None, out_rgba=None):
        """Meters the frame last rendered (weighted by what the eye looks at with abi.METER_GAZE), moves the renderer's exposure
        towards it and tone-maps the frame at that exposure, all on the device; cfg.mode = abi.EXPOSE_FIXED tone-maps at
        cfg.exposure and leaves the state alone.  in_color: device pointer of a float4 frame (None: the accum buffer; typically
        post_buffers()[0]).  out_color / out_rgba: device pointers (out_color may be in_color), or None for the renderer's own
        buffers (downloadExposedColor / downloadExposedPixels).  Enqueued on the renderer's stream, not synchronised (the
        downloads and expose_state() synchronise)."""
        cfg = cfg if cfg is not None else self.expose_defaults()
        self._check(self._L.fovpt_expose(self._ctx, C.byref(self.launchParams), C.byref(cfg), in_color, out_color, out_rgba))

    def expose_buffers(self):
        """Device addresses of the renderer's own exposed outputs: (float4 colour, rgba8)."""
        return self._own_buffers("expose")

    def expose_state(self) -> abi.ExposeState:
        """The exposure state after everything enqueued so far (synchronises the renderer's stream)."""
        s = abi.ExposeState()
        self._check(self._L.fovpt_expose_state(self._ctx, C.byref(s)))
        return s

    def expose_reset(self):
        """The next AUTO expose() is a first step: its exposure is the metered one."""
        self._check(self._L.fovpt_expose_reset(self._ctx))

    def downloadExposedPixels(self):
        """The rgba8 output of the last expose() into the renderer's own buffer, shaped like downloadPixels()."""
        return self._download_frame(self._own_buffers("expose")[1], 1)

    def downloadExposedColor(self):
        """The float4 output of the last expose() into the renderer's own buffer."""
        return self._download_frame(self._own_buffers("expose")[0], 4)

    # -- HDR glare ahead of the tone map (include/fovpt.h, fovpt_bloom)
    @staticmethod
    def bloom_defaults() -> abi.BloomConfig:
        return _defaults("bloom", abi.BloomConfig)

    def bloom(self, config=None, in_color=None, out_color=None, out_rgba=None):
        """Adds the glare of the frame's highlights to it, in HDR (fovpt_bloom): a bright pass whose threshold follows the exposure
        (config.flags & abi.BLOOM_EXPOSURE_STATE: the one expose() last adapted to, read on the device), a pyramid of
        config.levels levels, and the composite.  in_color: device pointer of a float4 frame (None: the accum buffer; typically
        focus_buffers()[0] or post_buffers()[0]), out_color / out_rgba: device pointers, or None for the renderer's own buffers
        (downloadBloomColor / downloadBloomPixels); out_color may be in_color.  Meant ahead of expose().  Enqueued on the
        renderer's stream, not synchronised (the downloads synchronise)."""
        config = config if config is not None else self.bloom_defaults()
        self._check(self._L.fovpt_bloom(self._ctx, C.byref(self.launchParams), C.byref(config), in_color, out_color, out_rgba))

    def bloomBuffers(self):
        """Device addresses of the renderer's own bloom outputs: (float4 colour, rgba8)."""
        return self._own_buffers("bloom")

    bloom_buffers = bloomBuffers               # the spelling of every other stage

    def downloadBloomPixels(self):
        """The rgba8 output of the last bloom() into the renderer's own buffer, shaped like downloadPixels()."""
        return self._download_frame(self._own_buffers("bloom")[1], 1)

    def downloadBloomColor(self):
        """The float4 output of the last bloom() into the renderer's own buffer."""
        return self._download_frame(self._own_buffers("bloom")[0], 4)

    # -- late reprojection of the finished frame to a newer camera (include/fovpt.h, fovpt_warp)
    @staticmethod
    def warp_defaults() -> abi.WarpConfig:
        return _defaults("warp", abi.WarpConfig)

    @staticmethod
    def warp_camera(camera) -> abi.WarpCamera:
        """An abi.WarpCamera from a Camera (its aspect ratio as set), a dict of eye / U / V / W triples, an abi.WarpCamera or a
        launchParams.camera."""
        from .renderer import Camera           # (renderer imports this module, so not at the top)
        to = abi.WarpCamera()
        if isinstance(camera, Camera):
            to.U, to.V, to.W = camera.UVWFrame()
            to.eye.set(camera.eye())
        elif isinstance(camera, dict):
            for k in ("eye", "U", "V", "W"):
                getattr(to, k).set(camera[k])
        else:
            C.memmove(C.byref(to), C.byref(camera), C.sizeof(abi.WarpCamera))
        return to

    def warp(self, to, cfg=None, gbuffer=None, in_color=None, in_rgba=None, out_color=None, out_rgba=None, out_map=None):
        """Re-aims the frame last rendered at the camera `to` (what warp_camera() takes): a depth-tested forward scatter of its
        pixels and a fill of the holes, on the device; pixels are copied, never blended.  gbuffer: an abi.GBufferPtrs of the
        rendered frame (temporal_gbuffer() after a post() / temporal() step saves the trace), None: traced by the call.  in_color /
        in_rgba: device pointers of a float4 / rgba8 frame (None: the accum / frame buffer; typically expose_buffers()).
        out_color / out_rgba: device pointers, or None for the renderer's own buffers (downloadWarpedColor /
        downloadWarpedPixels); out_map: device pointer of a uint32 frame (source | class << 30) or None.  Enqueued on the
        renderer's stream, not synchronised (the downloads and warp_counts() synchronise)."""
        cfg = cfg if cfg is not None else self.warp_defaults()
        to = self.warp_camera(to)
        self._check(self._L.fovpt_warp(self._ctx, C.byref(self.launchParams), C.byref(to), C.byref(cfg), _ref(gbuffer),
                                       in_color, in_rgba, out_color, out_rgba, out_map))

    @staticmethod
    def warp_motion_defaults() -> abi.WarpMotionConfig:
        return _defaults("warp_motion", abi.WarpMotionConfig)

    def warp_motion(self, to, cfg=None, gbuffer=None, in_color=None, in_rgba=None, out_color=None, out_rgba=None, out_map=None):
        """warp() in which the meshes that moved in the interval the last temporal step ended (temporal(), temporal_motion() or
        post()) go on moving: their pixels are scattered cfg.advance intervals further along their own motion.  Everything else,
        the buffers and warp_counts() included, is warp()'s.  gbuffer: as warp()'s; the hit records that go with it are the
        renderer's last G-buffer trace, which must be of the frame last rendered and of the current geometry (the library checks)."""
        cfg = cfg if cfg is not None else self.warp_motion_defaults()
        to = self.warp_camera(to)
        self._check(self._L.fovpt_warp_motion(self._ctx, C.byref(self.launchParams), C.byref(to), C.byref(cfg),
                                              _ref(gbuffer), in_color, in_rgba, out_color, out_rgba, out_map))

    def warp_depth(self, size, depth, from_camera, to, cfg=None, in_color=None, in_rgba=None, out_color=None, out_rgba=None, out_map=None):
        """warp() for a client that holds no scene and no rendered frame: the source points are rebuilt from `depth`, a device
        pointer of size[0] x size[1] floats (depth along W, +inf the sky: what decodeDepthPacket writes), and from_camera, the
        camera they were rendered with (PacketDepthHeader.camera; anything warp_camera() takes).  Every enabled image needs its
        input and its output, device pointers of the caller's; warp_counts() reports this warp.  Enqueued on the renderer's stream."""
        cfg = cfg if cfg is not None else self.warp_defaults()
        frm, to = self.warp_camera(from_camera), self.warp_camera(to)
        self._check(self._L.fovpt_warp_depth(self._ctx, int(size[0]), int(size[1]), C.byref(frm), C.byref(to), C.byref(cfg), depth,
                                             in_color, in_rgba, out_color, out_rgba, out_map))

    def warp_buffers(self):
        """Device addresses of the renderer's own warped outputs: (float4 colour, rgba8)."""
        return self._own_buffers("warp")

    def warp_counts(self) -> abi.WarpCounts:
        """The counts of the last warp() (synchronises the renderer's stream); zeros before any."""
        s = abi.WarpCounts()
        self._check(self._L.fovpt_warp_counts(self._ctx, C.byref(s)))
        return s

    def temporal_gbuffer(self) -> abi.GBufferPtrs:
        """The G-buffer set the last temporal step (temporal(), temporal_motion(), post()) traced: the rendered frame's."""
        g = abi.GBufferPtrs()
        self._check(self._L.fovpt_temporal_gbuffer(self._ctx, C.byref(g)))
        return g

    def downloadWarpedPixels(self):
        """The rgba8 output of the last warp() into the renderer's own buffer, shaped like downloadPixels()."""
        return self._download_frame(self._own_buffers("warp")[1], 1)

    def downloadWarpedColor(self):
        """The float4 output of the last warp() into the renderer's own buffer."""
        return self._download_frame(self._own_buffers("warp")[0], 4)

    # -- gaze-metered focus distance and depth of field (include/fovpt.h, fovpt_focus)
    @staticmethod
    def focus_defaults() -> abi.FocusConfig:
        return _defaults("focus", abi.FocusConfig)

    def focus_strength(self, lens_radius) -> float:
        """cfg.strength of a thin lens of radius lens_radius (scene units) at the current camera and frame height: the blur
        radius in pixels per unit of |1 / t - 1 / focus|, lens_radius * (h / 2) * |W| / |V|.  Host only."""
        cam = self.launchParams.camera
        norm = lambda v: math.sqrt(float(v.x) ** 2 + float(v.y) ** 2 + float(v.z) ** 2)
        return float(lens_radius) * (self.launchParams.frame.size.y / 2.0) * norm(cam.W) / norm(cam.V)

    def focus(self, cfg=None, gbuffer=None, in_color=None, out_color=None, out_rgba=None, out_coc=None):
        """Meters the distance of what the eye looks at in the frame last rendered (the cfg.rank_permille rank of the hit
        distances inside the gaze disc), moves the renderer's focus towards it in 1 / distance and blurs the frame by a per-pixel
        radius cfg.strength * |1 / t - 1 / focus| (at most cfg.max_radius pixels), all on the device; cfg.mode = abi.FOCUS_FIXED
        focuses at cfg.focus_distance and leaves the state alone.  gbuffer: an abi.GBufferPtrs of the rendered frame
        (temporal_gbuffer() after a post() / temporal() step saves the trace), None: traced by the call.  in_color: device pointer
        of a float4 frame (None: the accum buffer; typically post_buffers()[0]).  out_color / out_rgba: device pointers, or None
        for the renderer's own buffers (downloadFocus); out_coc: device pointer of a float frame (the radii) or None.  Enqueued on
        the renderer's stream, not synchronised (downloadFocus and focus_state() synchronise)."""
        cfg = cfg if cfg is not None else self.focus_defaults()
        self._check(self._L.fovpt_focus(self._ctx, C.byref(self.launchParams), C.byref(cfg), _ref(gbuffer),
                                        in_color, out_color, out_rgba, out_coc))

    def focus_buffers(self):
        """Device addresses of the renderer's own focused outputs: (float4 colour, rgba8)."""
        return self._own_buffers("focus")

    def focus_state(self) -> abi.FocusState:
        """The focus state after everything enqueued so far (synchronises the renderer's stream); zeros before any AUTO step."""
        s = abi.FocusState()
        self._check(self._L.fovpt_focus_state(self._ctx, C.byref(s)))
        return s

    def focus_reset(self):
        """The next AUTO focus() is a first step: its focus is the metered one."""
        self._check(self._L.fovpt_focus_reset(self._ctx))

    def downloadFocus(self):
        """The outputs of the last focus() into the renderer's own buffers: ((H, W, 4) float32 colour, rgba8 shaped like
        downloadPixels())."""
        col, rgba = self._own_buffers("focus")
        return self._download_frame(col, 4), self._download_frame(rgba, 1)

    # -- head-mounted display lens pre-distortion with chromatic correction (include/fovpt.h, fovpt_lens)
    @staticmethod
    def lens_defaults() -> abi.LensConfig:
        return _defaults("lens", abi.LensConfig)

    @staticmethod
    def lens_for_frame(cfg, width, height) -> abi.LensConfig:
        """A copy of cfg fitted to a width x height frame: scale.y = height / width and src_scale.y = width / height (the lens is
        round, the NDC square is not), then both src_scale entries divided by f(1) = k0 + k1 + k2 + k3, so that the mid-point of the
        left and right edges maps to itself.  Host only."""
        c = cfg.copy()
        f1 = float(c.k[0]) + (float(c.k[1]) + (float(c.k[2]) + float(c.k[3])))
        c.scale[1] = float(height) / float(width)
        c.src_scale[1] = float(width) / float(height)
        c.src_scale[0] = float(c.src_scale[0]) / f1
        c.src_scale[1] = float(c.src_scale[1]) / f1
        return c

    def lens(self, cfg=None, to=None, in_color=None, out_color=None, out_rgba=None):
        """Pre-distorts the frame last rendered for a head-mounted display's lens: for every display pixel and colour channel the
        position cfg's radial polynomial (times cfg.chroma[c]) maps it to is read from in_color with cfg.filter, on the device.
        cfg None: lens_for_frame(lens_defaults()) of the frame's size.  to: a late camera (what warp_camera() takes) whose ROTATION
        re-aims the rays in the same gather, None: no re-aim.  in_color: device pointer of a float4 frame (None: the accum buffer;
        typically expose_buffers()[0]).  out_color / out_rgba: device pointers, or None for the renderer's own buffers
        (downloadLens).  Enqueued on the renderer's stream, not synchronised (downloadLens synchronises)."""
        if cfg is None:
            f = self.launchParams.frame
            cfg = self.lens_for_frame(self.lens_defaults(), f.size.x, f.size.y)
        to = self.warp_camera(to) if to is not None else None
        self._check(self._L.fovpt_lens(self._ctx, C.byref(self.launchParams), C.byref(cfg), _ref(to),
                                       in_color, out_color, out_rgba))

    def lens_buffers(self):
        """Device addresses of the renderer's own pre-distorted outputs: (float4 colour, rgba8)."""
        return self._own_buffers("lens")

    def downloadLens(self):
        """The outputs of the last lens() into the renderer's own buffers: ((H, W, 4) float32 colour, rgba8 shaped like
        downloadPixels())."""
        col, rgba = self._own_buffers("lens")
        return self._download_frame(col, 4), self._download_frame(rgba, 1)

    # -- luminance moment history and variance-guided a-trous filter (include/fovpt.h, fovpt_variance / fovpt_variance_filter)
    @staticmethod
    def variance_defaults() -> abi.VarianceConfig:
        return _defaults("variance", abi.VarianceConfig)

    def variance(self, cfg=None, gbuffer=None, in_sample=None, motion=None, out_variance=None):
        """One step of the luminance moment history of the frame last rendered, and its variance image (rel, var, mean, n) per pixel:
        the history is read where `motion` says the pixel was (device pointer of a float4 frame as temporal_motion() / post() write
        it; None: at the pixel itself), a short history takes a spatial estimate instead.  gbuffer: an abi.GBufferPtrs of the
        rendered frame (temporal_gbuffer() after a post() / temporal() step saves the trace), None: traced by the call.  in_sample:
        device pointer of a float4 frame (None: the accum buffer); out_variance: device pointer, or None for the renderer's own image
        (downloadVariance).  Enqueued on the renderer's stream, not synchronised."""
        cfg = cfg if cfg is not None else self.variance_defaults()
        self._check(self._L.fovpt_variance(self._ctx, C.byref(self.launchParams), C.byref(cfg), _ref(gbuffer),
                                           in_sample, motion, out_variance))

    def variance_buffers(self):
        """Device addresses of the renderer's own variance image and of the moment history the last variance() wrote."""
        return self._own_buffers("variance")

    def variance_reset(self):
        """The next variance() has no history."""
        self._check(self._L.fovpt_variance_reset(self._ctx))

    def downloadVariance(self):
        """((H, W, 4) float32 variance image (rel, var, mean, n), (H, W, 4) float32 moment history (M1, M2, n, z)) of the last
        variance() into the renderer's own image."""
        var, mom = self._own_buffers("variance")
        return self._download_frame(var, 4), self._download_frame(mom, 4)

    @staticmethod
    def variance_filter_defaults() -> abi.VarianceFilterConfig:
        return _defaults("variance_filter", abi.VarianceFilterConfig)

    def variance_filter(self, cfg=None, gbuffer=None, in_color=None, variance=None, out_color=None, out_rgba=None):
        """Filters in_color (device pointer of a float4 frame; None: the accum buffer; typically post_buffers()[0]) with an a-trous
        filter whose luminance edge-stop is scaled by `variance` (device pointer of a variance image; None: the renderer's own, from
        the last variance()) and whose normal and plane-distance stops read the G-buffer (as variance()).  out_color / out_rgba:
        device pointers, or None for the renderer's own buffers (downloadVarianceFiltered).  Enqueued, not synchronised."""
        cfg = cfg if cfg is not None else self.variance_filter_defaults()
        self._check(self._L.fovpt_variance_filter(self._ctx, C.byref(self.launchParams), C.byref(cfg), _ref(gbuffer),
                                                  in_color, variance, out_color, out_rgba))

    def variance_filter_buffers(self):
        """Device addresses of the renderer's own filtered outputs: (float4 colour, rgba8)."""
        return self._own_buffers("variance_filter")

    def downloadVarianceFiltered(self):
        """The outputs of the last variance_filter() into the renderer's own buffers: ((H, W, 4) float32 colour, rgba8 shaped like
        downloadPixels())."""
        col, rgba = self._own_buffers("variance_filter")
        return self._download_frame(col, 4), self._download_frame(rgba, 1)

    # -- image quality of the rendered frame (include/fovpt.h, fovpt_quality): per-level error, SSIM and eccentricity profile
    @staticmethod
    def quality_defaults() -> abi.QualityConfig:
        return _defaults("quality", abi.QualityConfig)

    @staticmethod
    def quality_scores(sums) -> dict:
        """The derived scores of an abi.QualitySums (fovpt_quality_mse / _psnr / _ssim, host only): {"mse": {class name: value, ...,
        "all": every class but unwritten}, "psnr": ..., "ssim": ..., "profile_mse": the 64 rings' mean squared error}; NaN where a
        class or ring is empty."""
        L = lib.load_loader()
        keys = list(enumerate(abi.QUALITY_CLASS_NAMES)) + [(-1, "all")]
        out = {what: {name: float(getattr(L, "fovpt_quality_" + what)(C.byref(sums), k)) for k, name in keys} for what in ("mse", "psnr", "ssim")}
        out["profile_mse"] = [float(s) / (3.0 * float(n)) if n else float("nan") for s, n in zip(sums.ring_sq_err, sums.ring_pixels)]
        return out

    @staticmethod
    def quality_score(sums, weights) -> float:
        """fovpt_quality_score: the mean squared error with the five classes weighted (fovea, middle, periphery, uniform, unwritten)."""
        w = (C.c_double * abi.QUALITY_CLASSES)(*[float(v) for v in weights])
        return float(lib.load_loader().fovpt_quality_score(C.byref(sums), w))

    def _quality_image(self, who, image):
        """A device pointer as it is; an (H, W) uint32 numpy image of the frame's size uploaded (kept until the next read)."""
        if image is None or isinstance(image, int):
            return image
        f = self.launchParams.frame
        a = np.ascontiguousarray(image)
        if a.dtype != np.uint32 or a.shape != (f.size.y, f.size.x):
            raise ValueError("%s: a host image must be a (%d, %d) uint32 array" % (who, f.size.y, f.size.x))
        t = self._device_tensor(lambda torch, dev: torch.from_numpy(a.view(np.int32)).to(dev))
        self._quality_keep.append(t)
        return t.data_ptr()

    def qualityAsync(self, ref_rgba, test_rgba=None, config=None, out_sums=None, out_class=None):
        """Enqueues one measurement of the frame last rendered on the renderer's stream, not synchronised: test_rgba (None: the
        frame buffer) against ref_rgba, each a device pointer of an rgba8 image of the frame's size or an (H, W) uint32 numpy array.
        config None: quality_defaults().  out_sums: device pointer of an abi.QualitySums record, None: the renderer's own
        (readQuality); with records of the caller's any number of measurements may be in flight.  out_class: device pointer of one
        byte per pixel for the pixels' classes, or None."""
        cfg = config if config is not None else self.quality_defaults()
        ref, test = self._quality_image("qualityAsync", ref_rgba), self._quality_image("qualityAsync", test_rgba)
        self._check(self._L.fovpt_quality(self._ctx, C.byref(self.launchParams), C.byref(cfg), test, ref, out_sums, out_class))

    def readQuality(self, sums=False):
        """Waits for the renderer's stream and returns the renderer's own record as a dict: the fields of abi.QualitySums as Python
        integers and lists, and the derived scores of quality_scores().  sums=True: the abi.QualitySums itself."""
        s = abi.QualitySums()
        self._check(self._L.fovpt_quality_read(self._ctx, C.byref(s)))
        self._quality_keep = []
        if sums:
            return s
        out = s.as_dict()
        out.update(self.quality_scores(s))
        return out

    def measureQuality(self, ref_rgba, test_rgba=None, config=None, classes=False):
        """qualityAsync into the renderer's own record, then readQuality: the dict of the sums and the derived scores.
        classes=True: also "classes", the (H, W) uint8 class of every pixel (abi.QUALITY_FOVEA ..)."""
        cls = None
        if classes:
            f = self.launchParams.frame
            cls = self._device_tensor(lambda torch, dev: torch.zeros((f.size.y, f.size.x), dtype=torch.uint8, device=dev))
        self.qualityAsync(ref_rgba, test_rgba, config, None, cls.data_ptr() if cls is not None else None)
        out = self.readQuality()
        if cls is not None:
            out["classes"] = cls.cpu().numpy()
        return out

