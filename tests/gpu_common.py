"""General helpers of the GPU stage tests (test_*_gpu.py and the *_common.py modules of single stages): the box scene and its
renderers, views of a renderer's frame description, device buffers made and read through torch, "defaults with these entries
replaced", and the one way of building and running a drop-in program of tests/cpp/.  Nothing here belongs to one stage; what
does lives in that stage's *_common.py or in its test file.  Importing this module needs no GPU and no torch."""
import ctypes as C
import os
import subprocess

import numpy as np

import reconstruct_ref as rr
from fovpathtracing_optixcodelatest_amd import abi, scenes

from common import cfg_foveated, cfg_uniform, make_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the box scene ---------------------------------------------------------------------------------------------------------
def box_model(red_half=(1, 1, 1)):
    """A grey slab and a red box (half extents red_half): sky misses around them."""
    grey, red = abi.Material.reference_default(), abi.Material.reference_default()
    grey.color.set((0.7, 0.7, 0.7)); grey.emission.set((0, 0, 0))
    red.color.set((0.8, 0.1, 0.1)); red.emission.set((0, 0, 0))
    return scenes.Model([scenes.box_mesh((0, -1.0, 0), (6, 0.5, 6), grey), scenes.box_mesh((0, 0.5, 0), red_half, red)])


BOX_CAMERA = dict(eye=(4.0, 3.0, 6.0), lookat=(0.0, 0.5, 0.0), up=(0.0, 1.0, 0.0), fovy=45.0)


def box_renderer(size, cfg=None, gaze=None, write_guides=False, probe=None):
    """A renderer over the box scene seen from BOX_CAMERA.  cfg: default cfg_uniform(1); write_guides sets the flag in it;
    gaze: default the frame's centre; probe: default a 64 x 32 sky of 2.5."""
    cfg = cfg if cfg is not None else cfg_uniform(1)
    if write_guides:
        cfg.write_guides = 1
    return make_gpu(box_model(), probe if probe is not None else scenes.ambient_probe(64, 32, 2.5), BOX_CAMERA, size, cfg, gaze=gaze)


def dropin_renderer(write_guides=False, red_half=(1, 1, 1), **frame):
    """The python twin of tests/cpp/box_scene.h: BoxScene and its setup() -- 160 x 96, a 160 x 96 sky of 2.5, radii 12 / 36 at
    1 / 2 / 8 samples, the gaze at the centre, subframe 0 (frame: another gaze or subframe_index, as make_gpu takes them, where
    the program sets one after setup()).  The model is r.model.  Keep the two equal."""
    cfg = cfg_foveated(12, 36, (1, 2, 8))
    if write_guides:
        cfg.write_guides = 1
    return make_gpu(box_model(red_half), scenes.ambient_probe(160, 96, 2.5), BOX_CAMERA, (160, 96), cfg, **frame)


# ---- a renderer's frame description ------------------------------------------------------------------------------------------
def frame_size(r):
    f = r.launchParams.frame
    return f.size.x, f.size.y


def camera(r):
    """The launch parameters' camera as the restatements take it."""
    c = r.launchParams.camera
    vec = lambda v: (float(v.x), float(v.y), float(v.z))
    return dict(eye=vec(c.eye), U=vec(c.U), V=vec(c.V), W=vec(c.W))


def writer_fills(r):
    """(the fill of each pixel's last writer, the FOV_OFF flag) for the frame r rendered last: r.launchParams and r.config as
    at render time."""
    f, cfg = r.launchParams.frame, r.config
    return rr.writers(f.size.x, f.size.y, (f.c.x, f.c.y), cfg.r_inner, cfg.r_outer, cfg.uniform)[0], cfg.uniform


def debug_buffer(r, name):
    """(device address, bytes) of fovpt_debug_buffer(name); raises lib.FovptError like every call of the renderer."""
    p, n = C.c_void_p(), C.c_size_t()
    r._check(r._L.fovpt_debug_buffer(r._ctx, name.encode(), C.byref(p), C.byref(n)))
    return p.value, n.value


def with_entries(defaults, d=None):
    """A configuration struct as its fovpt_*_defaults made it, with the entries of d replaced -> the struct."""
    for k, v in (d or {}).items():
        setattr(defaults, k, v)
    return defaults


# ---- device buffers ------------------------------------------------------------------------------------------------------------
def upload(a):
    """The array on the device, as a torch tensor of its bytes: uint32 goes up viewed as int32 (torch uploads no uint32), every
    other dtype as it is.  Synchronised before it returns."""
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    torch.cuda.synchronize()
    return t


def device_filled(shape, fill=0x5a):
    """A uint8 device tensor of this shape (or, given a number, of that many bytes), every byte `fill`; synchronised."""
    import torch
    t = torch.full((shape,) if isinstance(shape, (int, np.integer)) else tuple(shape), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def device_images(size, *bytes_per_pixel, fill=0x5a):
    """One device_filled image of a frame of this size per entry: 16 for a float4 image, 4 for rgba8 and other words."""
    return [device_filled((size[1], size[0], b), fill) for b in bytes_per_pixel]


HOST_VIEWS = dict(color=(np.float32, 4), rgba=(np.uint32, None), map=(np.uint32, None), coc=(np.float32, None))


def host_view(t, kind):
    """A (H, W, bytes per pixel) device tensor on the host as the image it holds: "color" (H, W, 4) float32, "rgba" and "map"
    (H, W) uint32, "coc" (H, W) float32."""
    dtype, channels = HOST_VIEWS[kind]
    a = t.cpu().numpy().view(dtype)
    return a.reshape(a.shape[0], a.shape[1], channels) if channels else a.reshape(a.shape[0], a.shape[1])


# ---- the drop-in programs of tests/cpp/ ------------------------------------------------------------------------------------------
def build_dropin(tmp_path, name, extra=()):
    """Compiles tests/cpp/<name>.cpp against include/ and libfovpt.so -> the program's path under tmp_path.  extra: further
    arguments of the link."""
    exe = str(tmp_path / name)
    csrc = os.path.join(ROOT, "fovpathtracing_optixcodelatest_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", name + ".cpp"),
                           "-o", exe, "-L", csrc, "-lfovpt", "-Wl,-rpath," + csrc] + list(extra))
    return exe


def run_dropin(exe, *args):
    """Runs the program, 300 s at the most; a non-zero exit fails the test with what the program wrote -> the finished run."""
    res = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    return res
