"""Host-side mirror of the reference's renderer interface for the foveated launch path.

Same names, argument meaning and error behaviour as PT_sv5_/SimplePathtracer.h:45-72 and the
types it consumes (sutil::Camera, ProbeData), on top of the C ABI in include/fovpt.h.  All
compute happens in libfovpt.so (HIP, gfx950); nothing here touches pixels.
"""
import ctypes as C

import numpy as np

from . import abi, abi_depth, lib
from .api_animate import Animation
from .api_debug import DebugHooks
from .api_packet import Packets
from .api_post import PostStages
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


def decode_depth_packet(packet, size=None, out=None):
    """A depth packet (bytes-like, what waitPacket returned for a submitDepthPacket) -> the (H, W) float32 depth image along
    the rendered camera's W, +inf the sky (fovpt_packet_decode_depth_host); abi_depth.PacketDepthHeader.from_packet(packet)
    has the camera.  size, out: as decode_packet's, out a float32 array (None: zeros).  Needs the host-only loader library
    alone.  Raises lib.FovptError on bytes that are not a valid depth packet."""
    buf = bytes(packet)
    L = lib.load_loader()
    if size is None:
        if len(buf) < C.sizeof(abi_depth.PacketDepthHeader):
            raise lib.FovptError(-1, "decode_depth_packet: fewer than 192 bytes")
        h = abi_depth.PacketDepthHeader.from_packet(buf).base
        size = (h.width, h.height)
    w, h = int(size[0]), int(size[1])
    if out is None:
        if not (0 < w <= 16384 and 0 < h <= 16384):
            raise lib.FovptError(-1, "decode_depth_packet: width / height outside 1 .. 16384")
        out = np.zeros((h, w), np.float32)
    elif out.shape != (h, w) or out.dtype != np.float32 or not out.flags["C_CONTIGUOUS"]:
        raise ValueError("decode_depth_packet: out must be a C-contiguous (%d, %d) float32 array" % (h, w))
    lib.check(None, L.fovpt_packet_decode_depth_host(buf, len(buf), out.ctypes.data, w, h), L)
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


class SampleRenderer(PostStages, Packets, Animation, DebugHooks):
    """class SampleRenderer, PT_sv5_/SimplePathtracer.h:45-188 (public part).  Here: construction, plumbing, the reference's
    interface and the multi-GPU gather; the post-frame stages, the packets, animated geometry and the test hooks are the four
    parts api_post.py, api_packet.py, api_animate.py and api_debug.py, each beside the csrc/ file of the same name."""

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
        self._quality_keep = []                # host images qualityAsync uploaded, until readQuality
        self._keep_updates = []                # device tensors of the last device update, read on the stream after the call

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

