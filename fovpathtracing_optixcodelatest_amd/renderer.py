"""Host-side mirror of the reference's renderer interface for the foveated launch path.

Same names, argument meaning and error behaviour as PT_sv5_/SimplePathtracer.h:45-72 and the
types it consumes (sutil::Camera, ProbeData), on top of the C ABI in include/fovpt.h.  All
compute happens in libfovpt.so (HIP, gfx950); nothing here touches pixels.
"""
import ctypes as C
import math

import numpy as np

from . import abi, lib
from .scenes import Model, pack_model


def decode_packet(data, mode=abi.PACKET_NEAREST, size=None, out=None):
    """A foveated frame packet (bytes-like, e.g. what waitPacket returned on the rendering machine) -> the (H, W) uint32 rgba8
    image, abi.PACKET_NEAREST or abi.PACKET_SMOOTH (fovpt_packet_decode_host).  size: the (width, height) the caller expects
    (None: the packet's); out: an (H, W) uint32 array to decode into -- pixels no texel reaches keep their contents -- or None
    for a zeroed one.  Needs the host-only loader library alone: no GPU, no HIP runtime.  Raises lib.FovptError on bytes that
    are not a valid packet."""
    buf = bytes(data)
    L = lib.load_loader()
    if size is None:
        if len(buf) < C.sizeof(abi.PacketHeader):
            raise lib.FovptError(-1, "decode_packet: fewer than 128 bytes")
        h = abi.PacketHeader.from_packet(buf)
        size = (h.width, h.height)
    w, h = int(size[0]), int(size[1])
    if out is None:
        if not (0 < w <= 16384 and 0 < h <= 16384):
            raise lib.FovptError(-1, "decode_packet: width / height outside 1 .. 16384")
        out = np.zeros((h, w), np.uint32)
    elif out.shape != (h, w) or out.dtype != np.uint32 or not out.flags["C_CONTIGUOUS"]:
        raise ValueError("decode_packet: out must be a C-contiguous (%d, %d) uint32 array" % (h, w))
    lib.check(None, L.fovpt_packet_decode_host(buf, len(buf), int(mode), out.ctypes.data, w, h), L)
    return out


class Camera:
    """sutil::Camera (sutil/Camera.h:40-100): eye, lookat, up, fovY (degrees), aspect ratio."""

    def __init__(self, eye=(1.0, 1.0, 1.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fovY=35.0, aspectRatio=1.0):
        self.m_eye, self.m_lookat, self.m_up = tuple(eye), tuple(lookat), tuple(up)
        self.m_fovY, self.m_aspectRatio = float(fovY), float(aspectRatio)

    def eye(self):
        return self.m_eye

    def setEye(self, v):
        self.m_eye = tuple(v)

    def setAspectRatio(self, a):
        self.m_aspectRatio = float(a)

    def UVWFrame(self):
        """sutil/Camera.cpp:32-44, evaluated by the library's host helper."""
        e, l, u = abi.Float3().set(self.m_eye), abi.Float3().set(self.m_lookat), abi.Float3().set(self.m_up)
        U, V, W = abi.Float3(), abi.Float3(), abi.Float3()
        rc = lib.load().fovpt_camera_uvw(C.byref(e), C.byref(l), C.byref(u), self.m_fovY, self.m_aspectRatio,
                                         C.byref(U), C.byref(V), C.byref(W))
        lib.check(None, rc)
        return U, V, W


class ProbeData:
    """PT_sv5_/Probe.h:7-86.  data: (H,W,4) float32; BuildCDF() fills the four tables."""

    def __init__(self, data=None):
        self.valid = False
        self.offset = (0.0, 0.0, 0.0)
        self.data = None
        self.width = self.height = 0
        if data is not None:
            self.data = np.ascontiguousarray(data, np.float32)
            self.height, self.width = self.data.shape[:2]

    def BuildCDF(self):
        h, w = self.height, self.width
        self.pdfValuesX = np.empty((h, w), np.float32)
        self.cdfValuesX = np.empty((h, w), np.float32)
        self.pdfValuesY = np.empty(h, np.float32)
        self.cdfValuesY = np.empty(h, np.float32)
        rc = lib.load().fovpt_probe_build_cdf(w, h, self.data.ctypes.data, self.pdfValuesX.ctypes.data,
                                              self.cdfValuesX.ctypes.data, self.pdfValuesY.ctypes.data,
                                              self.cdfValuesY.ctypes.data)
        lib.check(None, rc)
        self.valid = True
        return self


class OutputBuffer:
    """Shape of sutil::CUDAOutputBuffer<uint32_t> (sutil/CUDAOutputBuffer.h:54-94): anything with
    map() -> device pointer of W*H uint32 and unmap().  Wraps a caller-owned device pointer."""

    def __init__(self, device_ptr):
        self._p = int(device_ptr)

    def map(self):
        return self._p

    def unmap(self):
        pass


class SampleRenderer:
    """class SampleRenderer, PT_sv5_/SimplePathtracer.h:45-188 (public part)."""

    def __init__(self, model: Model, device: int = 0):
        self._L = lib.load()
        self._ctx = C.c_void_p()
        lib.check(None, self._L.fovpt_create(C.byref(self._ctx), device))
        self.launchParams = abi.LaunchParams()
        self.model = model
        md, n, td, nt, keep = pack_model(model)
        trav = C.c_uint64()
        self._check(self._L.fovpt_set_scene(self._ctx, C.cast(md, C.c_void_p), n, C.cast(td, C.c_void_p), nt, C.byref(trav)))
        self.launchParams.traversable = trav.value                      # SimplePathtracer.cpp:61
        self.lastSetCamera = Camera()
        self._frame_ptrs = abi.FramePtrs()
        self._device = int(device)
        self._motion = None

    # -- plumbing -----------------------------------------------------------------------
    def _check(self, rc):
        lib.check(self._ctx, rc)

    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._L.fovpt_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return self._L.fovpt_stream(self._ctx)

    @property
    def config(self) -> abi.Config:
        c = abi.Config()
        self._check(self._L.fovpt_get_config(self._ctx, C.byref(c)))
        return c

    @config.setter
    def config(self, c: abi.Config):
        self._check(self._L.fovpt_set_config(self._ctx, C.byref(c)))

    def stats(self) -> abi.Stats:
        s = abi.Stats()
        self._check(self._L.fovpt_get_stats(self._ctx, C.byref(s)))
        return s

    def reset_stats(self):
        self._check(self._L.fovpt_reset_stats(self._ctx))

    def synchronize(self):
        self._check(self._L.fovpt_synchronize(self._ctx))

    # -- the reference's public interface ---------------------------------------------------
    def render(self, target=None):
        """render() / render(CUDAOutputBuffer&), SimplePathtracer.cpp:77-226.  Like the reference,
        render(target) repoints launchParams.frame.frame_buffer at the mapped target and leaves it
        there (:218-219).  Synchronises before returning (CUDA_SYNC_CHECK, :212)."""
        if target is not None:
            self.launchParams.frame.frame_buffer = target.map()
        self._check(self._L.fovpt_render(self._ctx, C.byref(self.launchParams)))
        self.synchronize()
        if target is not None:
            target.unmap()

    def render_async(self):
        """render() without the trailing synchronisation (for back-to-back timed frames)."""
        self._check(self._L.fovpt_render(self._ctx, C.byref(self.launchParams)))

    # -- multi-GPU gather of the owned pixels (include/fovpt.h, fovpt_gather_*) -------------
    def gather_plan(self):
        """Partition of the frame's pixels by owning rank for the current config / frame size / gaze -> counts per rank."""
        world = max(1, self.config.world)
        counts = (C.c_uint32 * world)()
        self._check(self._L.fovpt_gather_plan(self._ctx, C.byref(self.launchParams), counts, world))
        return [int(x) for x in counts]

    def gather_pack(self, frame_ptr, packed_ptr):
        self._check(self._L.fovpt_gather_pack(self._ctx, frame_ptr, packed_ptr))

    def gather_unpack(self, gathered_ptr, stride, frame_ptr):
        self._check(self._L.fovpt_gather_unpack(self._ctx, gathered_ptr, stride, frame_ptr))

    # -- the RCCL transport of that gather inside the library (fovpt_comm_*, fovpt_gather_frame): what a C++ host uses
    @staticmethod
    def comm_unique_id():
        lib.share_torch_rccl()
        buf = C.create_string_buffer(128)
        lib.check(None, lib.load().fovpt_comm_get_unique_id(buf))
        return buf.raw

    def comm_init(self, unique_id, rank, world):
        lib.share_torch_rccl()
        self._check(self._L.fovpt_comm_init(self._ctx, C.c_char_p(unique_id), rank, world))

    def comm_destroy(self):
        self._check(self._L.fovpt_comm_destroy(self._ctx))

    def gather_frame(self, root, frame_ptr, full_frame_ptr):
        self._check(self._L.fovpt_gather_frame(self._ctx, C.byref(self.launchParams), root, frame_ptr, full_frame_ptr))

    def launch(self, width, height):
        """One optixLaunch with the current launchParams (SimplePathtracer.cpp:148-157)."""
        self._check(self._L.fovpt_launch(self._ctx, C.byref(self.launchParams), width, height))

    def resize(self, newSize):
        """SimplePathtracer.cpp:228-274."""
        w, h = int(newSize[0]), int(newSize[1])
        if w == 0 or h == 0:
            return
        self._check(self._L.fovpt_resize(self._ctx, w, h, C.byref(self._frame_ptrs)))
        f = self.launchParams.frame
        f.size.x, f.size.y = w, h
        f.frame_buffer = self._frame_ptrs.frame_buffer
        f.accum_buffer = self._frame_ptrs.accum_buffer
        f.normal_buffer = self._frame_ptrs.normal_buffer
        f.color_buffer = self._frame_ptrs.color_buffer
        f.albedo_buffer = self._frame_ptrs.albedo_buffer

    def downloadPixels(self):
        """SimplePathtracer.cpp:276-280: always the renderer's own frame_buffer."""
        return self._download_frame(self._frame_ptrs.frame_buffer, 1)

    def downloadAccum(self):
        """The float4 accum_buffer (per-pixel radiance), the quantity parity is judged on."""
        return self._download_frame(self.launchParams.frame.accum_buffer, 4)

    def download(self, device_ptr, array):
        self._check(self._L.fovpt_download(self._ctx, device_ptr, array.ctypes.data, array.nbytes))
        return array

    def _download_frame(self, device_ptr, channels):
        """A per-pixel device buffer of the current frame size: (H, W) uint32 for channels = 1 (rgba8), (H, W, channels) float32 otherwise."""
        f = self.launchParams.frame
        if channels == 1:
            return self.download(device_ptr, np.empty((f.size.y, f.size.x), np.uint32))
        return self.download(device_ptr, np.empty((f.size.y, f.size.x, channels), np.float32))

    # -- denoiser of the rendered frame (include/fovpt.h, fovpt_denoise): in place of the reference family's OptiXDenoiser
    @staticmethod
    def denoise_defaults() -> abi.DenoiseConfig:
        d = abi.DenoiseConfig()
        lib.check(None, lib.load().fovpt_denoise_defaults(C.byref(d)))
        return d

    def denoise(self, cfg=None, out_color=None, out_rgba=None):
        """Filters the frame last rendered (needs config.write_guides = 1).  out_color / out_rgba: device pointers (float4 /
        rgba8 per pixel), or None for the renderer's own buffers (downloadDenoisedColor / downloadDenoisedPixels).  Enqueued on
        the renderer's stream, not synchronised (the downloads synchronise)."""
        cfg = cfg if cfg is not None else self.denoise_defaults()
        self._check(self._L.fovpt_denoise(self._ctx, C.byref(self.launchParams), C.byref(cfg), out_color, out_rgba))

    def denoise_buffers(self):
        """Device addresses of the renderer's own denoiser outputs: (float4 colour, rgba8)."""
        col, rgba = C.c_void_p(), C.c_void_p()
        self._check(self._L.fovpt_denoise_buffers(self._ctx, C.byref(col), C.byref(rgba)))
        return col.value, rgba.value

    def downloadDenoisedPixels(self):
        """The rgba8 output of the last denoise into the renderer's own buffer, shaped like downloadPixels()."""
        return self._download_frame(self.denoise_buffers()[1], 1)

    def downloadDenoisedColor(self):
        """The float4 output of the last denoise into the renderer's own buffer."""
        return self._download_frame(self.denoise_buffers()[0], 4)

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
        d = abi.ReconstructConfig()
        lib.check(None, lib.load().fovpt_reconstruct_defaults(C.byref(d)))
        return d

    def reconstruct(self, cfg=None, in_color=None, out_color=None, out_rgba=None):
        """Reconstructs the block-filled pixels of the frame last rendered (remodulate = 1 needs config.write_guides = 1).
        in_color: device pointer of a float4 frame (None: the accum buffer; e.g. denoise_buffers()[0]).  out_color / out_rgba:
        device pointers, or None for the renderer's own buffers (downloadReconstructedColor / downloadReconstructedPixels).
        Enqueued on the renderer's stream, not synchronised (the downloads synchronise)."""
        cfg = cfg if cfg is not None else self.reconstruct_defaults()
        self._check(self._L.fovpt_reconstruct(self._ctx, C.byref(self.launchParams), C.byref(cfg), in_color, out_color, out_rgba))

    def reconstruct_buffers(self):
        """Device addresses of the renderer's own reconstruction outputs: (float4 colour, rgba8)."""
        col, rgba = C.c_void_p(), C.c_void_p()
        self._check(self._L.fovpt_reconstruct_buffers(self._ctx, C.byref(col), C.byref(rgba)))
        return col.value, rgba.value

    def downloadReconstructedPixels(self):
        """The rgba8 output of the last reconstruct into the renderer's own buffer, shaped like downloadPixels()."""
        return self._download_frame(self.reconstruct_buffers()[1], 1)

    def downloadReconstructedColor(self):
        """The float4 output of the last reconstruct into the renderer's own buffer."""
        return self._download_frame(self.reconstruct_buffers()[0], 4)

    # -- temporal reprojection of the frame history (include/fovpt.h, fovpt_temporal)
    @staticmethod
    def temporal_defaults() -> abi.TemporalConfig:
        d = abi.TemporalConfig()
        lib.check(None, lib.load().fovpt_temporal_defaults(C.byref(d)))
        return d

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
        col, rgba, hist = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self._L.fovpt_temporal_buffers(self._ctx, C.byref(col), C.byref(rgba), C.byref(hist)))
        return col.value, rgba.value, hist.value

    def temporal_reset(self):
        """Drops the frame history: the next temporal() step outputs its input."""
        self._check(self._L.fovpt_temporal_reset(self._ctx))

    def downloadTemporalPixels(self):
        """The rgba8 output of the last temporal step into the renderer's own buffer, shaped like downloadPixels()."""
        return self._download_frame(self.temporal_buffers()[1], 1)

    def downloadTemporalColor(self):
        """The float4 output of the last temporal step into the renderer's own buffer."""
        return self._download_frame(self.temporal_buffers()[0], 4)

    def downloadTemporalHistory(self):
        """The history the last temporal step wrote: (H, W, 4) float32, rgb its output colour, w the history length."""
        return self._download_frame(self.temporal_buffers()[2], 4)

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
        import torch
        f = self.launchParams.frame
        shape = (f.size.y, f.size.x, 4)
        if self._motion is None or tuple(self._motion.shape) != shape:
            self.synchronize()                 # (a step may still be writing the buffer this one replaces)
            self._motion = torch.zeros(shape, dtype=torch.float32, device="cuda:%d" % self._device)
            torch.cuda.synchronize(self._device)
        return self._motion.data_ptr()

    def downloadMotion(self):
        """The motion vectors the last temporal_motion(out_motion=motion_buffer()) wrote: (H, W, 4) float32."""
        return self._download_frame(self.motion_buffer(), 4)

    # -- the post-frame chain in one call (include/fovpt.h, fovpt_post)
    @staticmethod
    def post_defaults() -> abi.PostConfig:
        d = abi.PostConfig()
        lib.check(None, lib.load().fovpt_post_defaults(C.byref(d)))
        return d

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
        col, rgba = C.c_void_p(), C.c_void_p()
        self._check(self._L.fovpt_post_buffers(self._ctx, C.byref(col), C.byref(rgba)))
        return col.value, rgba.value

    def downloadPostPixels(self):
        """The rgba8 output of the last post() into the renderer's own buffer, shaped like downloadPixels()."""
        return self._download_frame(self.post_buffers()[1], 1)

    def downloadPostColor(self):
        """The float4 output of the last post() into the renderer's own buffer."""
        return self._download_frame(self.post_buffers()[0], 4)

    # -- gaze-metered auto-exposure and tone map (include/fovpt.h, fovpt_expose)
    @staticmethod
    def expose_defaults() -> abi.ExposeConfig:
        d = abi.ExposeConfig()
        lib.check(None, lib.load().fovpt_expose_defaults(C.byref(d)))
        return d

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
        col, rgba = C.c_void_p(), C.c_void_p()
        self._check(self._L.fovpt_expose_buffers(self._ctx, C.byref(col), C.byref(rgba)))
        return col.value, rgba.value

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
        return self._download_frame(self.expose_buffers()[1], 1)

    def downloadExposedColor(self):
        """The float4 output of the last expose() into the renderer's own buffer."""
        return self._download_frame(self.expose_buffers()[0], 4)

    # -- HDR glare ahead of the tone map (include/fovpt.h, fovpt_bloom)
    @staticmethod
    def bloom_defaults() -> abi.BloomConfig:
        d = abi.BloomConfig()
        lib.check(None, lib.load().fovpt_bloom_defaults(C.byref(d)))
        return d

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
        col, rgba = C.c_void_p(), C.c_void_p()
        self._check(self._L.fovpt_bloom_buffers(self._ctx, C.byref(col), C.byref(rgba)))
        return col.value, rgba.value

    def downloadBloomPixels(self):
        """The rgba8 output of the last bloom() into the renderer's own buffer, shaped like downloadPixels()."""
        return self._download_frame(self.bloomBuffers()[1], 1)

    def downloadBloomColor(self):
        """The float4 output of the last bloom() into the renderer's own buffer."""
        return self._download_frame(self.bloomBuffers()[0], 4)

    # -- late reprojection of the finished frame to a newer camera (include/fovpt.h, fovpt_warp)
    @staticmethod
    def warp_defaults() -> abi.WarpConfig:
        d = abi.WarpConfig()
        lib.check(None, lib.load().fovpt_warp_defaults(C.byref(d)))
        return d

    @staticmethod
    def warp_camera(camera) -> abi.WarpCamera:
        """An abi.WarpCamera from a Camera (its aspect ratio as set), a dict of eye / U / V / W triples, an abi.WarpCamera or a
        launchParams.camera."""
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
        self._check(self._L.fovpt_warp(self._ctx, C.byref(self.launchParams), C.byref(to), C.byref(cfg), C.byref(gbuffer) if gbuffer is not None else None,
                                       in_color, in_rgba, out_color, out_rgba, out_map))

    @staticmethod
    def warp_motion_defaults() -> abi.WarpMotionConfig:
        d = abi.WarpMotionConfig()
        lib.check(None, lib.load().fovpt_warp_motion_defaults(C.byref(d)))
        return d

    def warp_motion(self, to, cfg=None, gbuffer=None, in_color=None, in_rgba=None, out_color=None, out_rgba=None, out_map=None):
        """warp() in which the meshes that moved in the interval the last temporal step ended (temporal(), temporal_motion() or
        post()) go on moving: their pixels are scattered cfg.advance intervals further along their own motion.  Everything else,
        the buffers and warp_counts() included, is warp()'s.  gbuffer: as warp()'s; the hit records that go with it are the
        renderer's last G-buffer trace, which must be of the frame last rendered and of the current geometry (the library checks)."""
        cfg = cfg if cfg is not None else self.warp_motion_defaults()
        to = self.warp_camera(to)
        self._check(self._L.fovpt_warp_motion(self._ctx, C.byref(self.launchParams), C.byref(to), C.byref(cfg),
                                              C.byref(gbuffer) if gbuffer is not None else None, in_color, in_rgba, out_color, out_rgba, out_map))

    def warp_buffers(self):
        """Device addresses of the renderer's own warped outputs: (float4 colour, rgba8)."""
        col, rgba = C.c_void_p(), C.c_void_p()
        self._check(self._L.fovpt_warp_buffers(self._ctx, C.byref(col), C.byref(rgba)))
        return col.value, rgba.value

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
        return self._download_frame(self.warp_buffers()[1], 1)

    def downloadWarpedColor(self):
        """The float4 output of the last warp() into the renderer's own buffer."""
        return self._download_frame(self.warp_buffers()[0], 4)

    # -- gaze-metered focus distance and depth of field (include/fovpt.h, fovpt_focus)
    @staticmethod
    def focus_defaults() -> abi.FocusConfig:
        d = abi.FocusConfig()
        lib.check(None, lib.load().fovpt_focus_defaults(C.byref(d)))
        return d

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
        self._check(self._L.fovpt_focus(self._ctx, C.byref(self.launchParams), C.byref(cfg), C.byref(gbuffer) if gbuffer is not None else None,
                                        in_color, out_color, out_rgba, out_coc))

    def focus_buffers(self):
        """Device addresses of the renderer's own focused outputs: (float4 colour, rgba8)."""
        col, rgba = C.c_void_p(), C.c_void_p()
        self._check(self._L.fovpt_focus_buffers(self._ctx, C.byref(col), C.byref(rgba)))
        return col.value, rgba.value

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
        col, rgba = self.focus_buffers()
        return self._download_frame(col, 4), self._download_frame(rgba, 1)

    # -- head-mounted display lens pre-distortion with chromatic correction (include/fovpt.h, fovpt_lens)
    @staticmethod
    def lens_defaults() -> abi.LensConfig:
        d = abi.LensConfig()
        lib.check(None, lib.load().fovpt_lens_defaults(C.byref(d)))
        return d

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
        self._check(self._L.fovpt_lens(self._ctx, C.byref(self.launchParams), C.byref(cfg), C.byref(to) if to is not None else None,
                                       in_color, out_color, out_rgba))

    def lens_buffers(self):
        """Device addresses of the renderer's own pre-distorted outputs: (float4 colour, rgba8)."""
        col, rgba = C.c_void_p(), C.c_void_p()
        self._check(self._L.fovpt_lens_buffers(self._ctx, C.byref(col), C.byref(rgba)))
        return col.value, rgba.value

    def downloadLens(self):
        """The outputs of the last lens() into the renderer's own buffers: ((H, W, 4) float32 colour, rgba8 shaped like
        downloadPixels())."""
        col, rgba = self.lens_buffers()
        return self._download_frame(col, 4), self._download_frame(rgba, 1)

    # -- luminance moment history and variance-guided a-trous filter (include/fovpt.h, fovpt_variance / fovpt_variance_filter)
    @staticmethod
    def variance_defaults() -> abi.VarianceConfig:
        d = abi.VarianceConfig()
        lib.check(None, lib.load().fovpt_variance_defaults(C.byref(d)))
        return d

    def variance(self, cfg=None, gbuffer=None, in_sample=None, motion=None, out_variance=None):
        """One step of the luminance moment history of the frame last rendered, and its variance image (rel, var, mean, n) per pixel:
        the history is read where `motion` says the pixel was (device pointer of a float4 frame as temporal_motion() / post() write
        it; None: at the pixel itself), a short history takes a spatial estimate instead.  gbuffer: an abi.GBufferPtrs of the
        rendered frame (temporal_gbuffer() after a post() / temporal() step saves the trace), None: traced by the call.  in_sample:
        device pointer of a float4 frame (None: the accum buffer); out_variance: device pointer, or None for the renderer's own image
        (downloadVariance).  Enqueued on the renderer's stream, not synchronised."""
        cfg = cfg if cfg is not None else self.variance_defaults()
        self._check(self._L.fovpt_variance(self._ctx, C.byref(self.launchParams), C.byref(cfg), C.byref(gbuffer) if gbuffer is not None else None,
                                           in_sample, motion, out_variance))

    def variance_buffers(self):
        """Device addresses of the renderer's own variance image and of the moment history the last variance() wrote."""
        var, mom = C.c_void_p(), C.c_void_p()
        self._check(self._L.fovpt_variance_buffers(self._ctx, C.byref(var), C.byref(mom)))
        return var.value, mom.value

    def variance_reset(self):
        """The next variance() has no history."""
        self._check(self._L.fovpt_variance_reset(self._ctx))

    def downloadVariance(self):
        """((H, W, 4) float32 variance image (rel, var, mean, n), (H, W, 4) float32 moment history (M1, M2, n, z)) of the last
        variance() into the renderer's own image."""
        var, mom = self.variance_buffers()
        return self._download_frame(var, 4), self._download_frame(mom, 4)

    @staticmethod
    def variance_filter_defaults() -> abi.VarianceFilterConfig:
        d = abi.VarianceFilterConfig()
        lib.check(None, lib.load().fovpt_variance_filter_defaults(C.byref(d)))
        return d

    def variance_filter(self, cfg=None, gbuffer=None, in_color=None, variance=None, out_color=None, out_rgba=None):
        """Filters in_color (device pointer of a float4 frame; None: the accum buffer; typically post_buffers()[0]) with an a-trous
        filter whose luminance edge-stop is scaled by `variance` (device pointer of a variance image; None: the renderer's own, from
        the last variance()) and whose normal and plane-distance stops read the G-buffer (as variance()).  out_color / out_rgba:
        device pointers, or None for the renderer's own buffers (downloadVarianceFiltered).  Enqueued, not synchronised."""
        cfg = cfg if cfg is not None else self.variance_filter_defaults()
        self._check(self._L.fovpt_variance_filter(self._ctx, C.byref(self.launchParams), C.byref(cfg), C.byref(gbuffer) if gbuffer is not None else None,
                                                  in_color, variance, out_color, out_rgba))

    def variance_filter_buffers(self):
        """Device addresses of the renderer's own filtered outputs: (float4 colour, rgba8)."""
        col, rgba = C.c_void_p(), C.c_void_p()
        self._check(self._L.fovpt_variance_filter_buffers(self._ctx, C.byref(col), C.byref(rgba)))
        return col.value, rgba.value

    def downloadVarianceFiltered(self):
        """The outputs of the last variance_filter() into the renderer's own buffers: ((H, W, 4) float32 colour, rgba8 shaped like
        downloadPixels())."""
        col, rgba = self.variance_filter_buffers()
        return self._download_frame(col, 4), self._download_frame(rgba, 1)

    # -- image quality of the rendered frame (include/fovpt.h, fovpt_quality): per-level error, SSIM and eccentricity profile
    @staticmethod
    def quality_defaults() -> abi.QualityConfig:
        d = abi.QualityConfig()
        lib.check(None, lib.load().fovpt_quality_defaults(C.byref(d)))
        return d

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
        import torch
        f = self.launchParams.frame
        a = np.ascontiguousarray(image)
        if a.dtype != np.uint32 or a.shape != (f.size.y, f.size.x):
            raise ValueError("%s: a host image must be a (%d, %d) uint32 array" % (who, f.size.y, f.size.x))
        t = torch.from_numpy(a.view(np.int32)).to("cuda:%d" % self._device)
        torch.cuda.synchronize(self._device)
        self._quality_keep.append(t)
        return t.data_ptr()

    def qualityAsync(self, ref_rgba, test_rgba=None, config=None, out_sums=None, out_class=None):
        """Enqueues one measurement of the frame last rendered on the renderer's stream, not synchronised: test_rgba (None: the
        frame buffer) against ref_rgba, each a device pointer of an rgba8 image of the frame's size or an (H, W) uint32 numpy array.
        config None: quality_defaults().  out_sums: device pointer of an abi.QualitySums record, None: the renderer's own
        (readQuality); with records of the caller's any number of measurements may be in flight.  out_class: device pointer of one
        byte per pixel for the pixels' classes, or None."""
        if not hasattr(self, "_quality_keep"):
            self._quality_keep = []
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
            import torch
            f = self.launchParams.frame
            cls = torch.zeros((f.size.y, f.size.x), dtype=torch.uint8, device="cuda:%d" % self._device)
            torch.cuda.synchronize(self._device)
        self.qualityAsync(ref_rgba, test_rgba, config, None, cls.data_ptr() if cls is not None else None)
        out = self.readQuality()
        if cls is not None:
            out["classes"] = cls.cpu().numpy()
        return out

    # -- foveated frame packets (include/fovpt.h, fovpt_packet_*): a frame off the device, small and without stopping the renderer
    def packetConfig(self, codec=True) -> abi.PacketConfig:
        """The fovpt_packet_config of a codec= argument: True -> fovpt_packet_defaults (BC1 where a pass's fill is above 1), a
        sequence of up to three abi.PACKET_RAW / PACKET_BC1 / PACKET_BY_FILL -> those, per launch pass; an abi.PacketConfig as it is."""
        if isinstance(codec, abi.PacketConfig):
            return codec
        cfg = abi.PacketConfig()
        self._L.fovpt_packet_defaults(C.byref(cfg))
        if codec is not True:
            codec = [int(k) for k in codec]
            if len(codec) > 3:
                raise ValueError("codec: at most three passes")
            for p in range(3):
                cfg.codec[p] = codec[p] if p < len(codec) else 0
        return cfg

    def describePacket(self, sequence=0, codec=None) -> abi.PacketHeader:
        """The header encodePacket / submitPacket would write for the frame last rendered (host only); .bytes sizes a buffer.
        codec: None -> a raw "FVPK" packet; otherwise a coded "FVPC" one (packetConfig)."""
        h = abi.PacketHeader()
        if codec is None:
            self._check(self._L.fovpt_packet_describe(self._ctx, C.byref(self.launchParams), sequence, C.byref(h)))
        else:
            self._check(self._L.fovpt_packet_describe_coded(self._ctx, C.byref(self.launchParams), C.byref(self.packetConfig(codec)), sequence, C.byref(h)))
        return h

    def encodePacket(self, out_packet, sequence=0, in_rgba=None, codec=None) -> abi.PacketHeader:
        """Encodes the frame last rendered into out_packet, a device pointer with describePacket().bytes of room.  in_rgba: device
        pointer of an rgba8 image of the frame's size (post_buffers()[1], expose_buffers()[1], ...), None: the frame buffer.
        Enqueued on the renderer's stream, not synchronised.  Returns the header it writes."""
        h = self.describePacket(sequence, codec)
        if codec is None:
            self._check(self._L.fovpt_packet_encode(self._ctx, C.byref(self.launchParams), in_rgba, sequence, out_packet))
        else:
            self._check(self._L.fovpt_packet_encode_coded(self._ctx, C.byref(self.launchParams), C.byref(self.packetConfig(codec)), in_rgba, sequence, out_packet))
        return h

    def submitPacket(self, sequence=0, in_rgba=None, codec=None) -> int:
        """encodePacket into the next of abi.PACKET_SLOTS slots and an asynchronous copy to the slot's pinned host buffer: does
        not wait for the GPU (except for the slot's previous copy, if that is still running).  Returns the slot for waitPacket."""
        slot = C.c_int(-1)
        if codec is None:
            self._check(self._L.fovpt_packet_submit(self._ctx, C.byref(self.launchParams), in_rgba, sequence, C.byref(slot)))
        else:
            self._check(self._L.fovpt_packet_submit_coded(self._ctx, C.byref(self.launchParams), C.byref(self.packetConfig(codec)), in_rgba, sequence, C.byref(slot)))
        return slot.value

    def waitPacket(self, slot) -> bytes:
        """Waits for that slot's copy alone (later frames keep running) and returns the packet's bytes: what a client hands to
        decode_packet()."""
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._L.fovpt_packet_wait(self._ctx, slot, C.byref(p), C.byref(n)))
        return C.string_at(p.value, n.value)

    def decodePacket(self, header, packet, out_rgba, mode=abi.PACKET_NEAREST):
        """The device decoder: header an abi.PacketHeader (host), packet and out_rgba device pointers (out_rgba: the header's
        width x height rgba8 pixels; those no texel reaches keep their contents).  Enqueued on the renderer's stream."""
        self._check(self._L.fovpt_packet_decode(self._ctx, C.byref(header), packet, int(mode), out_rgba))

    # -- what update_vertices, update_skinned and update_morphed share
    @staticmethod
    def _all_device(who, values):
        """All host or all device: True when there are values and every one is a CUDA tensor; a mix raises ValueError."""
        on_device = [hasattr(v, "is_cuda") and bool(v.is_cuda) for v in values]
        if any(on_device) and not all(on_device):
            raise ValueError("%s: mixes host arrays and device tensors" % who)
        return bool(on_device) and all(on_device)

    @staticmethod
    def _host_palette(who, mesh, m, noun):
        """A (J, 3, 4) array, or a (J, 4, 4) one whose last rows are 0 0 0 1, as contiguous (J, 3, 4) float32."""
        m = np.asarray(m, np.float32)
        if m.ndim == 3 and m.shape[1:] == (4, 4):
            if not (m[:, 3] == np.float32([0, 0, 0, 1])).all():
                raise ValueError("%s: mesh %d: the last row of a (4, 4) matrix must be 0 0 0 1" % (who, mesh))
            m = m[:, :3]
        if m.ndim != 3 or m.shape[1:] != (3, 4):
            raise ValueError("%s: mesh %d needs a (J, 3, 4) or (J, 4, 4) %s" % (who, mesh, noun))
        return np.ascontiguousarray(m)

    @staticmethod
    def _device_palette(who, mesh, m):
        """The device pointer of a contiguous float32 (J, 3, 4) CUDA tensor."""
        import torch
        if m.dtype != torch.float32 or m.dim() != 3 or tuple(m.shape[1:]) != (3, 4) or not m.is_contiguous():
            raise ValueError("%s: mesh %d needs a contiguous (J, 3, 4) float32 tensor" % (who, mesh))
        return m.data_ptr()

    @staticmethod
    def _rebuild_flag(rebuild):
        """rebuild=False / True / "async" as FOVPT_UPDATE_* bits (True: synchronous; "async": beside the frames, rebuild_state())."""
        if isinstance(rebuild, str):
            if rebuild != "async":
                raise ValueError("rebuild is False, True or \"async\", not %r" % (rebuild,))
            return abi.UPDATE_REBUILD_ASYNC
        return abi.UPDATE_REBUILD if rebuild else 0

    def _update(self, fn, entries, num, device, rebuild, keep):
        self._check(fn(self._ctx, entries, num, (abi.UPDATE_DEVICE if device else 0) | self._rebuild_flag(rebuild)))
        if device:
            self._keep_updates = keep          # (the tensors are read on the stream after the call returns)

    # -- animated geometry (include/fovpt.h, fovpt_update_vertices): optixAccelBuild(OPERATION_UPDATE) over the same build inputs
    def update_vertices(self, updates, rebuild=False):
        """New vertex positions for meshes of the scene: updates maps a mesh index to an (n, 3) float32 numpy array, or to a
        CUDA torch tensor (device pointers, read in stream order on the renderer's stream: torch's writes of them must be ordered
        before the call).  All host or all device.  rebuild=False refits the hierarchy asynchronously; True builds it anew
        (synchronous).  The renderer's Model is not changed."""
        items = sorted(updates.items())
        device = self._all_device("update_vertices", updates.values())
        ups = (abi.VertexUpdate * max(1, len(items)))()
        keep = []
        for k, (mesh, v) in enumerate(items):
            if device:
                import torch
                if v.dtype != torch.float32 or v.dim() != 2 or v.shape[1] != 3:
                    raise ValueError("update_vertices: mesh %d needs an (n, 3) float32 tensor" % mesh)
                v = v.contiguous()
                ptr, n = v.data_ptr(), v.shape[0]
            else:
                v = np.ascontiguousarray(v, np.float32)
                if v.ndim != 2 or v.shape[1] != 3:
                    raise ValueError("update_vertices: mesh %d needs an (n, 3) array" % mesh)
                ptr, n = v.ctypes.data, v.shape[0]
            keep.append(v)
            ups[k].mesh, ups[k].num_vertices, ups[k].vertex = int(mesh), int(n), ptr
        self._update(self._L.fovpt_update_vertices, ups, len(items), device, rebuild, keep)

    # -- rigid motion and the cost of the refit tree (include/fovpt.h, fovpt_update_transforms / fovpt_hierarchy_cost)
    def update_transforms(self, transforms, rebuild=False):
        """Per-mesh affine transforms of the positions the scene was set with: transforms maps a mesh index to a (3, 4) array,
        or a (4, 4) one whose last row is 0 0 0 1 (ValueError otherwise).  Absolute, not cumulative; applied on the device, then
        update_vertices()' refit (or, rebuild=True, rebuild) with the same ordering.  The renderer's Model is not changed."""
        items = sorted(transforms.items())
        tfs = (abi.MeshTransform * max(1, len(items)))()
        for k, (mesh, m) in enumerate(items):
            m = np.asarray(m, np.float32)
            if m.shape == (4, 4):
                if not np.array_equal(m[3], np.float32([0, 0, 0, 1])):
                    raise ValueError("update_transforms: mesh %d: the last row of a (4, 4) matrix must be 0 0 0 1" % mesh)
                m = m[:3]
            if m.shape != (3, 4):
                raise ValueError("update_transforms: mesh %d needs a (3, 4) or (4, 4) matrix" % mesh)
            tfs[k].mesh = int(mesh)
            tfs[k].m[:] = [float(x) for x in m.reshape(-1)]
        self._check(self._L.fovpt_update_transforms(self._ctx, tfs, len(items), self._rebuild_flag(rebuild)))

    def rebuild_state(self, wait=False, adopt=False) -> abi.RebuildInfo:
        """The background rebuild an update with rebuild="async" starts (state REBUILD_IDLE / _BUILDING / _READY, the counters,
        last_error, snapshot_update, ms_build).  Never waits for the device.  wait=True waits until the state is not BUILDING;
        adopt=True makes a READY hierarchy the scene's now (otherwise the next update that enqueues something does)."""
        out = abi.RebuildInfo()
        self._check(self._L.fovpt_rebuild_state(self._ctx, (abi.REBUILD_WAIT if wait else 0) | (abi.REBUILD_ADOPT if adopt else 0), C.byref(out)))
        return out

    def hierarchy_cost(self, wait=False) -> abi.HierarchyCost:
        """The SAH cost of the hierarchy as built and as last measured on the device (built, current, updates, measured).  The
        first call switches watching on: every later refit is followed by a measurement.  wait=False never blocks and may lag
        (measured < updates); wait=True measures the present tree if need be and waits for it.  Rebuild when current / built
        passes your threshold."""
        out = abi.HierarchyCost()
        self._check(self._L.fovpt_hierarchy_cost(self._ctx, abi.COST_WAIT if wait else 0, C.byref(out)))
        return out

    # -- skinning (include/fovpt.h, fovpt_set_skins / fovpt_update_skinned)
    def set_skins(self, skins):
        """Sets, replaces or removes the skins of meshes: skins maps a mesh index to (joints (n, 4) uint16, weights (n, 4)
        float32), n the mesh's vertex count, or to None (remove).  The skin's joint count is the largest index used plus one; a
        third element, (joints, weights, num_joints), states it instead.  Weights are used as given, not normalised.  Set-up-time
        state of the scene: copied before the call returns, geometry does not move.  Bad shapes raise ValueError."""
        items = sorted(skins.items())
        sk = (abi.MeshSkin * max(1, len(items)))()
        keep = []
        for k, (mesh, jw) in enumerate(items):
            if not 0 <= int(mesh) < len(self.model.meshes):
                raise ValueError("set_skins: mesh %d of %d" % (mesh, len(self.model.meshes)))
            sk[k].mesh, sk[k].num_vertices = int(mesh), int(self.model.meshes[mesh].vertex.shape[0])
            if jw is None:
                continue
            j, w = jw[0], jw[1]
            j = np.asarray(j)
            if j.ndim != 2 or j.shape[1] != 4 or j.dtype.kind not in "ui" or (j.size and (j.min() < 0 or j.max() > 0xffff)):
                raise ValueError("set_skins: mesh %d needs (n, 4) joint indices that fit uint16" % mesh)
            j, w = np.ascontiguousarray(j, np.uint16), np.ascontiguousarray(w, np.float32)
            if w.shape != j.shape:
                raise ValueError("set_skins: mesh %d needs (n, 4) weights, one per joint index" % mesh)
            keep += [j, w]
            sk[k].num_vertices, sk[k].num_joints = j.shape[0], (int(jw[2]) if len(jw) > 2 else int(j.max()) + 1 if j.size else 1)
            sk[k].joints, sk[k].weights = j.ctypes.data, w.ctypes.data
        self._check(self._L.fovpt_set_skins(self._ctx, sk, len(items)))

    def update_skinned(self, poses, rebuild=False):
        """Poses of skinned meshes: poses maps a mesh index to its palette, a (J, 3, 4) array or a (J, 4, 4) one whose last rows
        are 0 0 0 1, or a contiguous float32 CUDA torch tensor (J, 3, 4) (read in stream order on the renderer's stream, not
        validated), J the joint count of the mesh's skin.  All host or all device.  Every vertex's rest position goes through the
        weighted sum of its four joints' matrices on the device; absolute, not cumulative; then update_vertices()' refit (or,
        rebuild=True, rebuild) with the same ordering.  Bad shapes raise ValueError.  The renderer's Model is not changed."""
        items = sorted(poses.items())
        device = self._all_device("update_skinned", poses.values())
        ps = (abi.SkinPose * max(1, len(items)))()
        keep = []
        for k, (mesh, m) in enumerate(items):
            if device:
                ptr = self._device_palette("update_skinned", mesh, m)
            else:
                m = self._host_palette("update_skinned", mesh, m, "array")
                ptr = m.ctypes.data
            keep.append(m)
            ps[k].mesh, ps[k].num_joints, ps[k].matrices = int(mesh), int(m.shape[0]), ptr
        self._update(self._L.fovpt_update_skinned, ps, len(items), device, rebuild, keep)

    # -- morph targets (include/fovpt.h, fovpt_set_morphs / fovpt_update_morphed)
    def set_morphs(self, morphs):
        """Sets, replaces or removes the morph targets of meshes: morphs maps a mesh index to a list of targets or to None
        (remove).  A target is a dense (n, 3) float32 array of deltas, n the mesh's vertex count, or a pair (index (k,) unsigned
        integers, strictly ascending, delta (k, 3) float32) that moves k of the vertices; k may be 0.  Set-up-time state of the
        scene: copied before the call returns, geometry does not move.  Bad shapes raise ValueError."""
        items = sorted(morphs.items())
        mm = (abi.MeshMorph * max(1, len(items)))()
        keep = []
        for k, (mesh, targets) in enumerate(items):
            if not 0 <= int(mesh) < len(self.model.meshes):
                raise ValueError("set_morphs: mesh %d of %d" % (mesh, len(self.model.meshes)))
            nv = int(self.model.meshes[mesh].vertex.shape[0])
            mm[k].mesh, mm[k].num_vertices = int(mesh), nv
            if targets is None:
                continue
            if len(targets) == 0:
                raise ValueError("set_morphs: mesh %d: an empty list of targets (None removes them)" % mesh)
            ts = (abi.MorphTarget * len(targets))()
            for t, target in enumerate(targets):
                if isinstance(target, tuple):
                    idx, d = np.asarray(target[0]), np.ascontiguousarray(target[1], np.float32).reshape(-1, 3)
                    if idx.ndim != 1 or (idx.size and (idx.dtype.kind not in "ui" or idx.min() < 0 or idx.max() > 0xffffffff)) or idx.shape[0] != d.shape[0]:
                        raise ValueError("set_morphs: mesh %d target %d needs (k,) vertex indices and (k, 3) deltas" % (mesh, t))
                    idx = np.ascontiguousarray(idx, np.uint32)
                    keep.append(idx)
                    ts[t].index = idx.ctypes.data
                else:
                    d = np.ascontiguousarray(target, np.float32)
                    if d.ndim != 2 or d.shape != (nv, 3):
                        raise ValueError("set_morphs: mesh %d target %d: a dense target needs (%d, 3) deltas" % (mesh, t, nv))
                keep.append(d)
                ts[t].count, ts[t].delta = d.shape[0], (d.ctypes.data if d.shape[0] else None)
            keep.append(ts)
            mm[k].num_targets, mm[k].targets = len(targets), ts
        self._check(self._L.fovpt_set_morphs(self._ctx, mm, len(items)))

    def update_morphed(self, poses, rebuild=False):
        """Poses of morphed meshes: poses maps a mesh index to its weights, a (T,) float32 array, T the mesh's target count, or to
        a pair (weights, palette) whose palette is what update_skinned() takes for the mesh's skin; or to contiguous float32 CUDA
        torch tensors, (T,) and (J, 3, 4) (read in stream order on the renderer's stream, not validated).  All host or all
        device.  Every vertex's rest position takes w[t] * delta of each of its targets whose weight is not zero, in ascending
        targets, and then goes through the skin where a palette is given; absolute, not cumulative; then update_vertices()'
        refit (or, rebuild=True, rebuild) with the same ordering.  Bad shapes raise ValueError.  The renderer's Model is not
        changed."""
        items = [(mesh, v if isinstance(v, tuple) else (v, None)) for mesh, v in sorted(poses.items())]
        device = self._all_device("update_morphed", [x for _, v in items for x in v if x is not None])
        ps = (abi.MorphPose * max(1, len(items)))()
        keep = []
        for k, (mesh, (w, m)) in enumerate(items):
            if device:
                import torch
                if w.dtype != torch.float32 or w.dim() != 1 or not w.is_contiguous():
                    raise ValueError("update_morphed: mesh %d needs a contiguous (T,) float32 tensor of weights" % mesh)
                wp, mp = w.data_ptr(), (None if m is None else self._device_palette("update_morphed", mesh, m))
            else:
                w = np.ascontiguousarray(w, np.float32)
                if w.ndim != 1:
                    raise ValueError("update_morphed: mesh %d needs a (T,) array of weights" % mesh)
                if m is not None:
                    m = self._host_palette("update_morphed", mesh, m, "palette")
                wp, mp = w.ctypes.data, (None if m is None else m.ctypes.data)
            keep += [w, m]
            ps[k].mesh, ps[k].num_targets, ps[k].weights = int(mesh), int(w.shape[0]), wp
            ps[k].num_joints, ps[k].matrices = (0 if m is None else int(m.shape[0])), mp
        self._update(self._L.fovpt_update_morphed, ps, len(items), device, rebuild, keep)

    # -- rigs (include/fovpt.h, fovpt_set_rig / fovpt_update_animated)
    @staticmethod
    def pack_rig(rig):
        """(abi.RigDesc, what it points to) of a rig: a dict with parent (N,) integers, translation (N, 3), rotation (N, 4)
        (x y z w) and scale (N, 3) float32, the nodes' parents and rest poses; bindings, a list of dicts with mesh and either
        node (rigid), or joint_nodes (J,) and inverse_bind (J, 3, 4), or neither (morph weights only); clips, a list of lists of
        channels, each a dict with target, path and interpolation (abi.RIG_*), times (K,) and values (K, 3 / 4 / 3 / targets).
        Bad shapes raise ValueError; the values themselves are the library's to check."""
        keep = []

        def arr(a, dtype, shape, what):
            a = np.ascontiguousarray(a, dtype)
            if a.ndim != len(shape) or any(s is not None and s != d for s, d in zip(shape, a.shape)):
                raise ValueError("set_rig: %s needs shape %s, not %s" % (what, shape, a.shape))
            keep.append(a)
            return a

        parent = arr(rig["parent"], np.int32, (None,), "parent")
        n = parent.shape[0]
        t, q, s = arr(rig["translation"], np.float32, (n, 3), "translation"), arr(rig["rotation"], np.float32, (n, 4), "rotation"), \
            arr(rig["scale"], np.float32, (n, 3), "scale")
        nodes = (abi.RigNode * max(1, n))()
        for i in range(n):
            nodes[i].parent = int(parent[i])
            nodes[i].translation[:], nodes[i].rotation[:], nodes[i].scale[:] = t[i].tolist(), q[i].tolist(), s[i].tolist()
        bindings = list(rig.get("bindings", ()))
        bs = (abi.RigBinding * max(1, len(bindings)))()
        for k, b in enumerate(bindings):
            bs[k].mesh, bs[k].node = int(b["mesh"]), int(b.get("node", -1))
            if b.get("joint_nodes") is not None:
                j = np.asarray(b["joint_nodes"])
                if j.ndim != 1 or j.dtype.kind not in "ui" or (j.size and (j.min() < 0 or j.max() > 0xffff)):
                    raise ValueError("set_rig: binding %d needs (J,) joint nodes that fit uint16" % k)
                j = arr(j, np.uint16, (None,), "joint_nodes")
                ib = SampleRenderer._host_palette("set_rig", int(b["mesh"]), b["inverse_bind"], "inverse bind palette")
                if ib.shape[0] != j.shape[0]:
                    raise ValueError("set_rig: binding %d needs one inverse bind matrix per joint node" % k)
                keep.append(ib)
                bs[k].num_joints, bs[k].joint_nodes, bs[k].inverse_bind = j.shape[0], j.ctypes.data, ib.ctypes.data
        clips = list(rig.get("clips", ()))
        cs = (abi.RigClip * max(1, len(clips)))()
        for k, clip in enumerate(clips):
            ch = (abi.RigChannel * max(1, len(clip)))()
            for h, c in enumerate(clip):
                times = arr(c["times"], np.float32, (None,), "clip %d channel %d: times" % (k, h))
                values = arr(c["values"], np.float32, (times.shape[0], None), "clip %d channel %d: values" % (k, h))
                width = {abi.RIG_TRANSLATION: 3, abi.RIG_ROTATION: 4, abi.RIG_SCALE: 3}.get(int(c["path"]))
                if width is not None and values.shape[1] != width:
                    raise ValueError("set_rig: clip %d channel %d needs (K, %d) values" % (k, h, width))
                ch[h].target, ch[h].path, ch[h].interpolation, ch[h].num_keys = int(c["target"]), int(c["path"]), int(c["interpolation"]), times.shape[0]
                ch[h].times, ch[h].values = times.ctypes.data, values.ctypes.data
            keep.append(ch)
            cs[k].num_channels, cs[k].channels = len(clip), ch
        desc = abi.RigDesc()
        desc.nodes, desc.num_nodes, desc.bindings, desc.num_bindings, desc.clips, desc.num_clips = nodes, n, bs, len(bindings), cs, len(clips)
        keep += [nodes, bs, cs]
        return desc, keep

    def set_rig(self, rig):
        """Sets, replaces or (None) removes the scene's rig: see pack_rig() for the form.  Called after set_skins() / set_morphs(),
        either of which drops it.  Set-up-time state of the scene: copied before the call returns, geometry does not move."""
        if rig is None:
            self._check(self._L.fovpt_set_rig(self._ctx, None))
            return
        desc, keep = self.pack_rig(rig)
        self._check(self._L.fovpt_set_rig(self._ctx, C.byref(desc)))
        del keep

    def update_animated(self, clip, time, rebuild=False):
        """Poses every mesh the rig binds from clip `clip` at `time`: the keys are sampled, the hierarchy composed and the
        palettes, weights and rigid matrices applied on the device; absolute, not cumulative; then update_vertices()' refit (or,
        rebuild=True, rebuild) with the same ordering.  The caller wraps its own time to loop.  The renderer's Model is not
        changed."""
        self._check(self._L.fovpt_update_animated(self._ctx, int(clip), float(time), self._rebuild_flag(rebuild)))

    def setCamera(self, camera: Camera):
        """SimplePathtracer.cpp:282-289: aspect ratio is recomputed from the frame size."""
        self.lastSetCamera = camera
        f = self.launchParams.frame
        self.lastSetCamera.setAspectRatio(f.size.x / float(f.size.y) if f.size.y else 1.0)
        U, V, W = self.lastSetCamera.UVWFrame()
        cam = self.launchParams.camera
        cam.U, cam.V, cam.W = U, V, W
        cam.eye.set(self.lastSetCamera.eye())

    def setCameraFov(self, eye, forward, up, angle_left, angle_right, angle_up, angle_down):
        """Per-eye asymmetric frustum from OpenXR-style half angles (XrFovf, radians; left/down negative), as the
        VR callers of the path compute them (OtherProjects_01/11HelloRaytracingOpenXR/main.cpp:891-897).  The raygen
        maps d in [-1,1]^2 to dir = d.x*U + d.y*V + W (deviceProgram.cu:483-491), so an off-centre frustum is W
        shifted by the tangent-space centre and U, V scaled by the tangent-space half extents."""
        f = np.array(forward, np.float64)
        f = f / np.linalg.norm(f)
        r_ = np.cross(f, np.array(up, np.float64))
        r_ = r_ / np.linalg.norm(r_)
        u = np.cross(r_, f)
        tl, tr, tu, td = (float(np.tan(a)) for a in (angle_left, angle_right, angle_up, angle_down))
        cam = self.launchParams.camera
        cam.eye.set(eye)
        cam.U.set((0.5 * (tr - tl)) * r_)
        cam.V.set((0.5 * (tu - td)) * u)
        cam.W.set(f + (0.5 * (tr + tl)) * r_ + (0.5 * (tu + td)) * u)

    def setProbe(self, probe: ProbeData):
        """SimplePathtracer.cpp:292-308; raises like CUDAProbeData::createBuffer (Probe.h:104-105)."""
        if not probe.valid:
            raise RuntimeError("Probe Data is not valid")
        off = abi.Float3().set(probe.offset)
        out = abi.Probe()
        self._check(self._L.fovpt_set_probe(self._ctx, probe.width, probe.height, probe.data.ctypes.data,
                                            probe.pdfValuesX.ctypes.data, probe.cdfValuesX.ctypes.data,
                                            probe.pdfValuesY.ctypes.data, probe.cdfValuesY.ctypes.data,
                                            C.byref(off), C.byref(out)))
        self.launchParams.probe = out

    def setProbeData(self, data, offset=(0.0, 0.0, 0.0)):
        """loadColor / loadProbe + BuildCDF + setProbe in one step (main.cpp:161-187, 306), with BuildCDF
        run on the device (fovpt_set_probe_data).  Returns the device-side tables for inspection."""
        data = np.ascontiguousarray(data, np.float32)
        h, w = data.shape[:2]
        off = abi.Float3().set(offset)
        out = abi.Probe()
        self._check(self._L.fovpt_set_probe_data(self._ctx, w, h, data.ctypes.data, C.byref(off), C.byref(out)))
        self.launchParams.probe = out
        return out

    def debug_trace(self, origins, dirs):
        """The production traversal kernel on a batch of rays -> (global prim id or 0xffffffff, (t, u, v), occluded 0 / 1)."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = o.shape[0]
        prim, tuv, occ = np.empty(n, np.uint32), np.empty((n, 3), np.float32), np.empty(n, np.uint8)
        self._check(self._L.fovpt_debug_trace(self._ctx, n, o.ctypes.data, d.ctypes.data, prim.ctypes.data, tuv.ctypes.data, occ.ctypes.data))
        return prim, tuv, occ

    def debug_trace_queued(self, rays, q_count, sq_count, sel=0, it_closest=0, it_shadow=0, grid_closest=0, grid_shadow=0, slots=0,
                           decoy=None, other=None, both=False):
        """The production traversal launches (closest hit, then occlusion) on a queue state laid out here (include/fovpt.h,
        fovpt_debug_trace_queued).  rays = dict(o (n, 3), d (n, 3), slot (n,), target (n,), vis (n, 4), occ (n, 4)); q_count /
        sq_count (8,) = the rays per shard of the radiance / shadow queue; other = the other chain's rays with q_count and
        sq_count among its keys (sel != 0 only); both: run the other chain's launches behind this one's.
        -> dict: cap; hit = dict(shard, pos, rec (k, 4) float32, prim) of the hit-buffer entries found, in ascending physical
        order; hit_found; cells (N + 1, max_depth, 4) and alpha (N + 1, 4) float32 of all N = n + n_other slots and the trap
        slot, the fill pattern abi.DEBUG_SHADE_FILL where nothing was written; stat_radiance, stat_shadow, stat_paths (what the
        launches added); counters_changed; queues_unchanged."""
        L = abi.DebugTraceLaunch()
        keep = []                                                   # (the arrays the struct points into)

        def put(prefix, r):
            o = np.ascontiguousarray(r["o"], np.float32).reshape(-1, 3)
            k = o.shape[0]
            a = dict(origins3=o, dirs3=np.ascontiguousarray(r["d"], np.float32).reshape(k, 3),
                     slot=np.ascontiguousarray(r["slot"], np.uint32).reshape(k), target=np.ascontiguousarray(r["target"], np.uint32).reshape(k),
                     vis4=np.ascontiguousarray(r["vis"], np.float32).reshape(k, 4), occ4=np.ascontiguousarray(r["occ"], np.float32).reshape(k, 4))
            for key, arr in a.items():
                keep.append(arr)
                setattr(L, prefix + key, arr.ctypes.data)
            return k

        n = put("", rays)
        m = put("other_", other) if other is not None else 0
        L.n, L.n_other, L.sel, L.both = n, m, sel, 1 if both else 0
        L.it_closest, L.it_shadow, L.grid_closest, L.grid_shadow, L.slots = it_closest, it_shadow, grid_closest, grid_shadow, slots
        for s in range(8):
            L.q_count[s], L.sq_count[s] = int(q_count[s]), int(sq_count[s])
            L.other_q_count[s] = int(other["q_count"][s]) if other is not None else 0
            L.other_sq_count[s] = int(other["sq_count"][s]) if other is not None else 0
            L.decoy[s] = int(decoy[s]) if decoy is not None else 0
        N, depth = n + m, self.config.max_depth
        a = dict(hit_place2=np.empty((N, 2), np.uint32), hit4=np.empty((N, 4), np.float32), hit_prim=np.empty(N, np.uint32),
                 cells4=np.empty((N + 1, depth, 4), np.float32), alpha4=np.empty((N + 1, 4), np.float32))
        R = abi.DebugTraceResult()
        for k, v in a.items():
            v.view(np.uint8)[...] = abi.DEBUG_SHADE_FILL
            setattr(R, k, v.ctypes.data)
        self._check(self._L.fovpt_debug_trace_queued(self._ctx, C.byref(L), C.byref(R)))
        k = min(int(R.hit_found), N)
        return dict(cap=int(R.cap), hit=dict(shard=a["hit_place2"][:k, 0], pos=a["hit_place2"][:k, 1], rec=a["hit4"][:k], prim=a["hit_prim"][:k]),
                    hit_found=int(R.hit_found), cells=a["cells4"], alpha=a["alpha4"], stat_radiance=int(R.stat_radiance),
                    stat_shadow=int(R.stat_shadow), stat_paths=int(R.stat_paths), counters_changed=int(R.counters_changed),
                    queues_unchanged=int(R.queues_unchanged))

    def debug_probe_sample(self, r12, plain=False, probe=None):
        """The production probe_sample with its two random numbers given (pairs in [0, 0.999999]) on `probe` (default: the launch
        parameters' probe), searched the way a launch would, or plainly -> dict(row, col, dir, color, pdf, path): path = the
        abi.PROBE_PATH_* bits of the layout that ran."""
        r = np.ascontiguousarray(r12, np.float32).reshape(-1, 2)
        n = r.shape[0]
        rowcol, out, path = np.empty((n, 2), np.int32), np.empty((n, 7), np.float32), C.c_int(0)
        self._check(self._L.fovpt_debug_probe_sample(self._ctx, C.byref(probe if probe is not None else self.launchParams.probe),
                                                     abi.DEBUG_PROBE_PLAIN if plain else 0, n, r.ctypes.data, rowcol.ctypes.data,
                                                     out.ctypes.data, C.byref(path)))
        return dict(row=rowcol[:, 0].copy(), col=rowcol[:, 1].copy(), dir=out[:, 0:3].copy(), color=out[:, 3:6].copy(),
                    pdf=out[:, 6].copy(), path=path.value)

    def debug_probe_eval(self, dirs, plain=False, probe=None):
        """probe_dir_to_uv + probe_eval, the backplate of a camera ray -> dict(uv, texel, path)."""
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = d.shape[0]
        out, path = np.empty((n, 6), np.float32), C.c_int(0)
        self._check(self._L.fovpt_debug_probe_eval(self._ctx, C.byref(probe if probe is not None else self.launchParams.probe),
                                                   abi.DEBUG_PROBE_PLAIN if plain else 0, n, d.ctypes.data, out.ctypes.data, C.byref(path)))
        return dict(uv=out[:, 0:2].copy(), texel=out[:, 2:6].copy(), path=path.value)

    def debug_bsdf(self, material, N, view, albedo, etaI, etaO, seeds, L_given):
        """Per row: bsdf_sample with Random(seed), bsdf_eval / bsdf_pdf at the sampled direction when its pdf is above 0, and
        bsdf_pdf / bsdf_eval at L_given -> the columns of oracle.bsdf_table_given (without `type`)."""
        N, view, albedo, L_given = (np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in (N, view, albedo, L_given))
        etaI, etaO = np.ascontiguousarray(etaI, np.float32), np.ascontiguousarray(etaO, np.float32)
        seeds = np.ascontiguousarray(seeds, np.int32)
        n = N.shape[0]
        assert view.shape[0] == albedo.shape[0] == L_given.shape[0] == etaI.size == etaO.size == seeds.size == n
        out = np.empty((n, 14), np.float32)
        self._check(self._L.fovpt_debug_bsdf(self._ctx, C.byref(material), n, N.ctypes.data, view.ctypes.data, albedo.ctypes.data,
                                             etaI.ctypes.data, etaO.ctypes.data, seeds.ctypes.data, L_given.ctypes.data, out.ctypes.data))
        return dict(light=out[:, 0:3].copy(), pdf=out[:, 3].copy(), eval=out[:, 4:7].copy(), pdf_again=out[:, 7].copy(),
                    rng_after=out[:, 8:10].copy().view(np.uint32), eval_given=out[:, 10:13].copy(), pdf_given=out[:, 13].copy())

    def debug_tex2d(self, texture, uv):
        """tex2d of texture `texture` of the scene at (u, v) pairs -> (n, 4) float32."""
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        out = np.empty((uv.shape[0], 4), np.float32)
        self._check(self._L.fovpt_debug_tex2d(self._ctx, int(texture), uv.shape[0], uv.ctypes.data, out.ctypes.data))
        return out

    def debug_shade(self, origin, dir4, prim, tuv, rng3, thr4, depth_iter=0, sel=0, grid=1, partition=0, shard_count=None, probe=None):
        """The production k_shade on n chosen hits, one launch under the current config (max_depth, options, write_guides) ->
        dict: per slot rng (n, 4) uint32, thr, rad (n, max_depth, 4), alpha, guide_n, guide_a (float32; the fill pattern where
        nothing was written); next_count / shadow_count (8,); next / shadow = dict(shard, pos, o, d[, vis, occ]) of the queue
        entries found, in ascending physical order; next_found / shadow_found, counters_changed, cap."""
        o = np.ascontiguousarray(origin, np.float32).reshape(-1, 3)
        n = o.shape[0]
        d = np.ascontiguousarray(dir4, np.float32).reshape(n, 4)
        prim = np.ascontiguousarray(prim, np.uint32).reshape(n)
        tuv = np.ascontiguousarray(tuv, np.float32).reshape(n, 3)
        rng3 = np.ascontiguousarray(rng3, np.uint32).reshape(n, 3)
        thr4 = np.ascontiguousarray(thr4, np.float32).reshape(n, 4)
        depth = self.config.max_depth
        L = abi.DebugShadeLaunch()
        L.n, L.depth_iter, L.grid, L.partition, L.sel = n, depth_iter, grid, partition, sel
        if shard_count is None:
            shard_count = [0] * 8
            shard_count[4 if sel == 2 else 0] = n
        for s in range(8):
            L.shard_count[s] = int(shard_count[s])
        f4 = lambda *shape: np.empty(shape + (4,), np.float32)
        a = dict(rng4=np.empty((n, 4), np.uint32), thr4=f4(n), rad4=f4(n, depth), alpha4=f4(n), guide_n4=f4(n), guide_a4=f4(n),
                 next_place2=np.empty((n, 2), np.uint32), next_o4=f4(n), next_d4=f4(n), shadow_place2=np.empty((n, 2), np.uint32),
                 shadow_o4=f4(n), shadow_d4=f4(n), shadow_vis4=f4(n), shadow_occ4=f4(n))
        for v in a.values():
            v.view(np.uint8)[...] = abi.DEBUG_SHADE_FILL
        R = abi.DebugShadeResult()
        for k, v in a.items():
            setattr(R, k, v.ctypes.data)
        self._check(self._L.fovpt_debug_shade(self._ctx, C.byref(probe if probe is not None else self.launchParams.probe), C.byref(L),
                                              o.ctypes.data, d.ctypes.data, prim.ctypes.data, tuv.ctypes.data, rng3.ctypes.data, thr4.ctypes.data,
                                              C.byref(R)))
        nn, ns = min(R.next_found, n), min(R.shadow_found, n)
        return dict(rng=a["rng4"], thr=a["thr4"], rad=a["rad4"], alpha=a["alpha4"], guide_n=a["guide_n4"], guide_a=a["guide_a4"],
                    next_count=np.array(R.next_count[:], np.uint32), shadow_count=np.array(R.shadow_count[:], np.uint32),
                    next=dict(shard=a["next_place2"][:nn, 0], pos=a["next_place2"][:nn, 1], o=a["next_o4"][:nn], d=a["next_d4"][:nn]),
                    shadow=dict(shard=a["shadow_place2"][:ns, 0], pos=a["shadow_place2"][:ns, 1], o=a["shadow_o4"][:ns], d=a["shadow_d4"][:ns],
                                vis=a["shadow_vis4"][:ns], occ=a["shadow_occ4"][:ns]),
                    next_found=int(R.next_found), shadow_found=int(R.shadow_found), counters_changed=int(R.counters_changed), cap=int(R.cap))

    def debug_build(self, tri, mesh_of_prim=None, ploc=True, split_budget=0.0, reinsert_rounds=0, order_children=True):
        """The production hierarchy build over `tri` (T, 9) float32 under explicit switches, and what every stage left -> dict of
        the arrays and scalars of struct fovpt_debug_build_trace (include/fovpt.h), the arrays cut to the build's sizes; an array
        its build did not make (no splits, a tiny build) is None.  Touches neither the scene nor the environment."""
        tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 9)
        n = tri.shape[0]
        mesh = None if mesh_of_prim is None else np.ascontiguousarray(mesh_of_prim, np.uint32).reshape(n)
        sw = abi.DebugBuildSwitches(1 if ploc else 0, float(split_budget), int(reinsert_rounds), 1 if order_children else 0)
        cap, rounds = int(n * (1.0 + float(split_budget))) + 1, 4097
        ci = max(cap - 1, 1)
        u32, i32, f32 = np.uint32, np.int32, np.float32
        a = dict(split_count=np.zeros(n, u32), split_first=np.zeros(n, u32), ref_prim=np.zeros(cap, u32), boxes=np.zeros((cap, 6), f32),
                 keys_s=np.zeros(cap, np.uint64), vals_s=np.zeros(cap, u32), left0=np.zeros(ci, i32), right0=np.zeros(ci, i32),
                 ibox0=np.zeros((ci, 6), f32), round_end=np.zeros(rounds, u32), left1=np.zeros(ci, i32), right1=np.zeros(ci, i32),
                 ibox1=np.zeros((ci, 6), f32), size_int=np.zeros(ci, u32), node_first=np.zeros(ci, u32), leaf_pos=np.zeros(cap, u32),
                 dp=np.zeros((ci, 4), u32), nodes_pre=np.zeros((ci, 32), u32), nodes=np.zeros((ci, 32), u32), tris=np.zeros((cap, 12), u32))
        T = abi.DebugBuildTrace()
        for k, v in a.items():
            setattr(T, k, v.ctypes.data)
        T.cap_refs, T.cap_rounds = cap, rounds
        self._check(self._L.fovpt_debug_build(self._ctx, n, tri.ctypes.data, mesh.ctypes.data if mesh is not None else None, C.byref(sw), C.byref(T)))
        R, N = int(T.num_refs), int(T.num_nodes)
        I = 0 if T.tiny else R - 1
        size = dict(split_count=n if T.have_count else None, split_first=n if T.have_splits else None, ref_prim=R if T.have_splits else None,
                    boxes=R, keys_s=None if T.tiny else R, vals_s=R, leaf_pos=R, round_end=int(T.num_rounds) if (ploc and not T.tiny) else None,
                    nodes_pre=N, nodes=N, tris=R)
        out = {}
        for k, v in a.items():
            m = size.get(k, None if T.tiny else I)
            out[k] = None if m is None else v[:m].copy()
        for k in ("num_refs", "tiny", "have_count", "have_splits", "root", "num_rounds", "num_nodes", "max_depth", "reinserted", "num_levels"):
            out[k] = int(getattr(T, k))
        out["s_cut"] = np.float32(T.s_cut)
        out["cbounds"] = np.array(T.cbounds[:], np.float32)
        out["level_first"] = [int(x) for x in T.level_first[:int(T.num_levels) + 1]]
        return out

    def debug_resolve_passes(self, render=True, width=0, height=0):
        """The pass table of the frame a render() (or a launch(width, height)) of the current launch parameters would resolve:
        a list of abi.DebugPass.  Sample slot of (pass, launch index li, sample s) = slot_base + li * spp + s."""
        passes, n = (abi.DebugPass * 3)(), C.c_int(0)
        self._check(self._L.fovpt_debug_resolve(self._ctx, C.byref(self.launchParams), 1 if render else 0, int(width), int(height), passes,
                                                C.byref(n), None, None, None, None, None, None, None))
        return [passes[i] for i in range(n.value)]

    def debug_resolve(self, state, cells, alpha, backplate, guide_n=None, guide_a=None, render=True, width=0, height=0):
        """The production resolve kernel on a path state in slot order (debug_resolve_passes): state (slots,) uint32 =
        flags | depth << 8, cells (slots, max_depth, 4), alpha (slots, 4), backplate (launch records, 4), guides (slots, 4) under
        write_guides.  The results are in the frame buffers (downloadAccum, downloadPixels, ...).  Returns the number of
        queue-counter words the kernel left non-zero."""
        passes = self.debug_resolve_passes(render, width, height)
        slots = sum(p.gw * p.rows * p.spp for p in passes)
        launches = sum(p.gw * p.rows for p in passes)
        depth = self.config.max_depth
        state = np.ascontiguousarray(state, np.uint32)
        cells, alpha, backplate = (np.ascontiguousarray(x, np.float32) for x in (cells, alpha, backplate))
        assert state.shape == (slots,) and cells.shape == (slots, depth, 4) and alpha.shape == (slots, 4) and backplate.shape == (launches, 4)
        guides = []
        for g in (guide_n, guide_a):
            if g is not None:
                g = np.ascontiguousarray(g, np.float32)
                assert g.shape == (slots, 4)
            guides.append(g)
        out, n, left = (abi.DebugPass * 3)(), C.c_int(0), C.c_uint32(0)
        self._check(self._L.fovpt_debug_resolve(self._ctx, C.byref(self.launchParams), 1 if render else 0, int(width), int(height), out, C.byref(n),
                                                state.ctypes.data, cells.ctypes.data, alpha.ctypes.data,
                                                guides[0].ctypes.data if guides[0] is not None else None,
                                                guides[1].ctypes.data if guides[1] is not None else None, backplate.ctypes.data, C.byref(left)))
        return left.value

    def debug_generate(self, render=True, width=0, height=0, rows=None, sel=0, slot_begin=0, slot_end=0, grid=0):
        """The production generate launch on the frame a render() (or a launch(width, height), or its chunk of launch rows
        rows = (row0, row1)) of the current launch parameters would run, as a job launches it: sel = 0 or a chain's 1 / 2, the
        sample slots [slot_begin, slot_end) (0, 0: a job's own), grid blocks (0: a job's own) -> dict: passes (list of
        abi.DebugPass), rng (slots, 4) uint32, backplate (launch records, 4), guide_n / guide_a (slots, 4) or None without
        write_guides -- the fill pattern abi.DEBUG_SHADE_FILL where nothing was written --, count (8,), found, counters_changed,
        cap, kernel (0 k_generate, 1 k_generate_owned), slot_begin, slot_end, grid as launched, and the queue entries found in
        ascending physical order: shard, pos, o (n, 4), d (n, 4)."""
        L = abi.DebugGenerateLaunch()
        L.render, L.width, L.height = 1 if render else 0, int(width), int(height)
        L.row0, L.row1 = (int(rows[0]), int(rows[1])) if rows is not None else (0, 0)
        L.sel, L.slot_begin, L.slot_end, L.grid = int(sel), int(slot_begin), int(slot_end), int(grid)
        passes, n = (abi.DebugPass * 3)(), C.c_int(0)
        self._check(self._L.fovpt_debug_generate(self._ctx, C.byref(self.launchParams), C.byref(L), passes, C.byref(n), None))
        table = [passes[i] for i in range(n.value)]
        slots = sum(p.gw * p.rows * p.spp for p in table)
        launches = sum(p.gw * p.rows for p in table)
        guides = bool(self.config.write_guides)
        a = dict(rng4=np.empty((slots, 4), np.uint32), backplate4=np.empty((launches, 4), np.float32), place2=np.empty((slots, 2), np.uint32),
                 o4=np.empty((slots, 4), np.float32), d4=np.empty((slots, 4), np.float32))
        if guides:
            a.update(guide_n4=np.empty((slots, 4), np.float32), guide_a4=np.empty((slots, 4), np.float32))
        R = abi.DebugGenerateResult()
        for k, v in a.items():
            v.view(np.uint8)[...] = abi.DEBUG_SHADE_FILL
            setattr(R, k, v.ctypes.data)
        self._check(self._L.fovpt_debug_generate(self._ctx, C.byref(self.launchParams), C.byref(L), passes, C.byref(n), C.byref(R)))
        assert bool(R.guides) == guides
        m = min(R.found, slots)
        return dict(passes=table, rng=a["rng4"], backplate=a["backplate4"], guide_n=a.get("guide_n4"), guide_a=a.get("guide_a4"),
                    count=np.array(R.count[:], np.uint32), found=int(R.found), counters_changed=int(R.counters_changed), cap=int(R.cap),
                    kernel=int(R.kernel), slot_begin=int(R.slot_begin), slot_end=int(R.slot_end), grid=int(R.grid),
                    shard=a["place2"][:m, 0], pos=a["place2"][:m, 1], o=a["o4"][:m], d=a["d4"][:m])

    def debug_math(self, op, a, b=None):
        a = np.ascontiguousarray(a, np.float32)
        bb = np.ascontiguousarray(b, np.float32) if b is not None else None
        out = np.empty_like(a)
        self._check(self._L.fovpt_debug_math(self._ctx, op, a.ctypes.data, bb.ctypes.data if bb is not None else None,
                                             out.ctypes.data, a.size))
        return out
