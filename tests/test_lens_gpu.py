"""fovpt_lens on the GPU against tests/lens_ref.py, bit for bit: the three filters with equal and with distinct chroma factors, with
and without a re-aim (a small turn, and a 120 degree turn that puts part of the frame behind the rendered camera), a barrel and a
pincushion polynomial, a finite clip radius, an off-centre axis, a non-black border and both encodes, at frame sizes from 1 x 1 up;
coefficients that overflow; the accum buffer as the input, the renderer's own buffers, reallocation; ordering with frames in flight;
every rejection; the C++ drop-in.  The input is synthetic colour uploaded by the test; the frame is a trivial render of the box scene.
The conditions that keep a case from being vacuous are asserted on the restatement's output."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import lens_ref as lr
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer

from common import cfg_foveated
from gpu_common import (BOX_CAMERA, bits, box_renderer, build_dropin, camera, device_images, dropin_renderer, host_view,
                        run_dropin, upload, with_entries)

pytestmark = pytest.mark.gpu
E_INVALID, E_NO_FRAME = -1, -5
SIZES = [(1, 1), (2, 1), (1, 3), (5, 4), (33, 17), (193, 109)]
FILTERS = (abi.LENS_NEAREST, abi.LENS_BILINEAR, abi.LENS_BICUBIC)
DISTINCT, EQUAL = (0.97, 1.0, 1.04), (1.014, 1.014, 1.014)
BORDER = (0.25, 0.5, 0.75, 0.5)
# what a case replaces in fovpt_lens_defaults fitted to the frame (lens_for_frame); `fit` False: the unfitted defaults
CASES = {
    "barrel": dict(),                                                     # the defaults' k = (1, 0.22, 0.24, 0): the corners read outside the source
    "pincushion": dict(k=(1.0, -0.15, 0.02, 0.0), fit=False),
    "clip": dict(clip_r2=0.8, border=BORDER),
    "off-centre": dict(center=(0.2, -0.1), src_center=(0.15, -0.05), encode=abi.LENS_ENCODE_RESOLVE),
    "border": dict(border=BORDER, src_scale_by=1.3, encode=abi.LENS_ENCODE_RESOLVE),
}


def lcfg(size, **d):
    """fovpt_lens_defaults, fitted to the frame unless fit=False, with the entries of d replaced -> (abi.LensConfig, the dict the
    restatement takes)."""
    d = dict(d)
    c = renderer.SampleRenderer.lens_defaults()
    if d.pop("fit", True):
        c = renderer.SampleRenderer.lens_for_frame(c, size[0], size[1])
    by = d.pop("src_scale_by", None)
    if by is not None:
        c.src_scale[0], c.src_scale[1] = c.src_scale[0] * by, c.src_scale[1] * by
    return with_entries(c, d), c.as_dict()


def turned(size, degrees):
    """BOX_CAMERA turned about its up axis by `degrees` (and moved: the re-aim ignores the eye) -> (abi.WarpCamera, dict)."""
    e, l = np.array(BOX_CAMERA["eye"], np.float64), np.array(BOX_CAMERA["lookat"], np.float64)
    a = math.radians(degrees)
    v = l - e
    v = np.array([math.cos(a) * v[0] + math.sin(a) * v[2], v[1], -math.sin(a) * v[0] + math.cos(a) * v[2]])
    eye = e + np.array([0.5, -0.25, 1.0])
    to = renderer.SampleRenderer.warp_camera(renderer.Camera(tuple(eye), tuple(eye + v), BOX_CAMERA["up"], BOX_CAMERA["fovy"], size[0] / float(size[1])))
    vec = lambda q: (float(q.x), float(q.y), float(q.z))
    return to, dict(eye=vec(to.eye), U=vec(to.U), V=vec(to.V), W=vec(to.W))


def synthetic(size, seed=0):
    w, h = size
    c = np.random.default_rng(seed).uniform(0.0, 1.5, (h, w, 4)).astype(np.float32)
    c[..., 3] = 0.5
    return c


def run(r, oracle, color, dev_color, cfg, full, to=None, label=None):
    """One fovpt_lens of the uploaded colour into caller's buffers, compared with the restatement -> the restatement's output."""
    f = r.launchParams.frame
    size = (f.size.x, f.size.y)
    oc, op = device_images(size, 16, 4)
    r.lens(cfg, to[0] if to else None, dev_color.data_ptr(), oc.data_ptr(), op.data_ptr())
    r.synchronize()
    want = lr.lens(oracle, color, full, camera(r), to[1] if to else None)
    n = lr.TAPS[full["filter"]] ** 2
    partly = (want["border_taps"] > 0) & (want["border_taps"] < n)
    x0, y0, ok = want["x0"], want["y0"], want["valid"].all(axis=-1)
    texel = [y0[..., c] * size[0] + x0[..., c] for c in range(3)]
    apart = ok & (texel[0] != texel[1]) & (texel[1] != texel[2]) & (texel[0] != texel[2])
    want["counts"] = dict(valid=int(want["valid"].sum()), invalid=int((~want["valid"]).sum()), outside_lens=int((~want["inside"]).sum()),
                          behind=int((~want["front"]).sum()),
                          partly_outside=int(partly.sum()), channels_apart=int(apart.sum()))
    print(label, want["counts"])
    assert np.array_equal(bits(host_view(oc, "color")), bits(want["color"])), label
    assert np.array_equal(host_view(op, "rgba"), want["rgba"]), label
    return want


# ---- 1. bit for bit --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_bit_for_bit(oracle, size):
    r = box_renderer(size)
    r.render()
    color = synthetic(size, size[0])
    dev = upload(color)
    tos = (None, turned(size, 2.0), turned(size, 120.0))
    names = list(CASES)
    seen = set()
    for i, (flt, chroma, to) in enumerate(itertools.product(FILTERS, (EQUAL, DISTINCT), tos)):
        for name in (names[i % 5], names[(i + 2) % 5]):
            cfg, full = lcfg(size, filter=flt, chroma=chroma, **CASES[name])
            want = run(r, oracle, color, dev, cfg, full, to, label=(size, flt, chroma == EQUAL, i % 3, name))
            seen.add((flt, name))
            if to is tos[2] and size[0] > 30:                              # part of the frame looks behind the rendered camera
                assert want["counts"]["behind"] > 0
    assert len(seen) == 15                                                # every case with every filter
    r.close()


@pytest.mark.parametrize("flt", FILTERS)
def test_the_cases_are_what_they_are_meant_to_be(oracle, flt):
    size = SIZES[-1]
    r = box_renderer(size)
    r.render()
    color = synthetic(size, 7)
    dev = upload(color)
    small, far = turned(size, 2.0), turned(size, 120.0)
    for name, d in CASES.items():
        cfg, full = lcfg(size, filter=flt, chroma=DISTINCT, **d)
        k = run(r, oracle, color, dev, cfg, full, small, label=(flt, name))["counts"]
        assert k["valid"] > 1000 and k["channels_apart"] > 0, (name, k)
        if name != "pincushion":
            assert k["invalid"] + k["outside_lens"] > 0, (name, k)
        if name == "clip":
            assert k["outside_lens"] > 100
        if flt != abi.LENS_NEAREST and name not in ("pincushion", "clip"):     # (the clip cuts the lens inside the source's edges)
            assert k["partly_outside"] > 0, (name, k)
    # the identity, and the shared lookup against three
    cfg, full = lcfg(size, filter=flt, k=(1.0, 0.0, 0.0, 0.0), chroma=(1.0, 1.0, 1.0), fit=False)
    want = run(r, oracle, color, dev, cfg, full, label=(flt, "identity"))
    if flt == abi.LENS_NEAREST:
        assert np.array_equal(bits(want["color"][..., :3]), bits(color[..., :3]))
    else:                                                                  # (fx is x to within its rounding: the neighbours' weights are not exactly 0)
        assert np.abs(want["color"][..., :3] - color[..., :3]).max() < 1e-3
    assert (want["color"][..., 3] == 1.0).all()
    cfg, full = lcfg(size, filter=flt, chroma=EQUAL, border=BORDER)
    want = run(r, oracle, color, dev, cfg, full, small, label=(flt, "equal"))
    each = lr.lens(oracle, color, full, camera(r), small[1], share=False)
    assert np.array_equal(bits(want["color"]), bits(each["color"])) and np.array_equal(want["rgba"], each["rgba"])
    # the 120 degree turn: part of the frame looks behind the rendered camera (a.z <= 0), the rest in front of it but far beside its
    # image (the two cameras' fields of view do not meet); a 50 degree turn keeps a part of the image
    k = run(r, oracle, color, dev, cfg, full, far, label=(flt, "120 degrees"))["counts"]
    assert k["behind"] > 100 and k["invalid"] - k["behind"] > 100 and k["valid"] == 0
    k = run(r, oracle, color, dev, cfg, full, turned(size, 50.0), label=(flt, "50 degrees"))["counts"]
    assert k["invalid"] > 100 and k["valid"] > 100 and k["partly_outside"] > (0 if flt != abi.LENS_NEAREST else -1)
    # coefficients that are valid but overflow: every channel invalid, the whole frame is the border
    cfg, full = lcfg(size, filter=flt, k=(1.0, 0.0, 0.0, 3e38), scale=(1000.0, 1000.0), center=(0.003, 0.003), border=BORDER)
    for to in (None, small):
        want = run(r, oracle, color, dev, cfg, full, to, label=(flt, "overflow"))
        assert want["counts"]["valid"] == 0
        assert (bits(want["color"][..., :3]) == bits(np.float32(BORDER[:3]))).all() and (want["color"][..., 3] == 1.0).all()
    r.close()


# ---- 2. the accum buffer, the renderer's own buffers, reallocation ---------------------------------------------------------------------
def test_the_accum_buffer_the_own_buffers_and_a_resize(oracle):
    small, large = (96, 64), (200, 120)
    r = box_renderer(small)
    with pytest.raises(lib.FovptError) as e:                 # nothing rendered yet
        r.lens()
    assert e.value.code == E_NO_FRAME
    with pytest.raises(lib.FovptError) as e:
        r.lens_buffers()
    assert e.value.code == E_NO_FRAME
    r.render()
    accum = r.downloadAccum()
    cfg, full = lcfg(small, filter=abi.LENS_BICUBIC, encode=abi.LENS_ENCODE_RESOLVE)
    oc, op = device_images(small, 16, 4)
    r.lens(cfg, None, None, oc.data_ptr(), op.data_ptr())    # in_color None: the accum buffer
    r.lens(cfg)                                              # and into the renderer's own buffers
    got_c, got_p = r.downloadLens()
    want = lr.lens(oracle, accum, full)
    assert np.array_equal(bits(got_c), bits(want["color"])) and np.array_equal(got_p, want["rgba"])
    assert np.array_equal(bits(host_view(oc, "color")), bits(got_c)) and np.array_equal(host_view(op, "rgba"), got_p)
    assert len(np.unique(got_p)) > 20 and np.array_equal(bits(r.downloadAccum()), bits(accum))
    before = r.lens_buffers()
    r.resize(large)
    r.setCamera(r.lastSetCamera)
    with pytest.raises(lib.FovptError) as e:                 # nothing rendered at this size yet
        r.lens()
    assert e.value.code == E_NO_FRAME
    r.render()
    accum = r.downloadAccum()
    r.lens()                                                 # the defaults fitted to the frame
    got_c, got_p = r.downloadLens()
    assert got_c.shape == (large[1], large[0], 4) and all(r.lens_buffers())
    want = lr.lens(oracle, accum, lcfg(large)[1])
    assert np.array_equal(bits(got_c), bits(want["color"])) and np.array_equal(got_p, want["rgba"])
    assert before[0] and before[1]
    r.close()


# ---- 3. ordering -----------------------------------------------------------------------------------------------------------------------
def test_lens_is_ordered_with_frames_in_flight():
    """render_async, lens, render_async, lens with no synchronisation in between: what the same sequence gives with a synchronise
    after every call.  A lens call issued right behind a render sees that render."""
    import torch
    size = (384, 216)
    cfg = cfg_foveated(20, 60, (4, 8, 16))
    cfg.frames_in_flight = 2
    r = box_renderer(size, cfg)
    lc, _ = lcfg(size, encode=abi.LENS_ENCODE_RESOLVE)
    views = [((190, 108), 0), ((300, 40), 1), ((80, 60), 2)]
    outs = [[device_images(size, 16, 4) for _ in views] for _ in range(2)]
    for sync, out in zip((True, False), outs):
        for g, k in views:                                   # the accum buffer's leftovers where no pass writes, as all views leave them
            r.launchParams.frame.c.x, r.launchParams.frame.c.y = g
            r.launchParams.frame.subframe_index = k
            r.render()
        for (g, k), (oc, op) in zip(views, out):
            r.launchParams.frame.c.x, r.launchParams.frame.c.y = g
            r.launchParams.frame.subframe_index = k
            r.render_async()
            if sync:
                r.synchronize()
            r.lens(lc, None, None, oc.data_ptr(), op.data_ptr())
            if sync:
                r.synchronize()
        r.synchronize()
    for want, got in zip(*outs):
        for x, y in zip(want, got):
            assert torch.equal(x, y)
    a, b = host_view(outs[0][0][1], "rgba"), host_view(outs[0][2][1], "rgba")
    assert (a != b).mean() > 0.1                             # (the frames differ: the comparison is not of copies)
    r.close()


# ---- 4. rejections ---------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_everything_unchanged():
    size = (96, 64)
    r = box_renderer(size)
    L = lib.load()
    good, _ = lcfg(size)
    with pytest.raises(lib.FovptError) as e:                 # nothing rendered yet
        r.lens(good)
    assert e.value.code == E_NO_FRAME
    r.render()
    oc, op = device_images(size, 16, 4)
    to, _ = turned(size, 2.0)
    r.lens(good, to, None, oc.data_ptr(), op.data_ptr())
    r.lens(good, to)
    r.synchronize()

    def everything():
        own = r.downloadLens()
        return (own[0].tobytes(), own[1].tobytes(), oc.cpu().numpy().tobytes(), op.cpu().numpy().tobytes())

    before = everything()
    outs = dict(out_color=oc.data_ptr(), out_rgba=op.data_ptr())

    def refuse(code, label, **kw):
        args = dict(cfg=good, to=to, in_color=None, **outs)
        args.update(kw)
        with pytest.raises(lib.FovptError) as e:
            r.lens(**args)
        assert e.value.code == code, label
        assert everything() == before, label

    def with_entry(name, i, v):
        c = good.copy()
        if i is None:
            setattr(c, name, v)
        else:
            getattr(c, name)[i] = v
        return c

    nan, inf = float("nan"), float("inf")
    for v in (-1, 3, 1 << 20):
        refuse(E_INVALID, ("filter", v), cfg=with_entry("filter", None, v))
    for v in (-1, 2, 1 << 20):
        refuse(E_INVALID, ("encode", v), cfg=with_entry("encode", None, v))
    for name, n in (("_reserved0", 2), ("_reserved", 8)):
        for i in range(n):
            refuse(E_INVALID, (name, i), cfg=with_entry(name, i, 1))
    for name, n in (("center", 2), ("scale", 2), ("k", 4), ("chroma", 3), ("src_center", 2), ("src_scale", 2), ("border", 4)):
        for i in range(n):
            for v in (nan, inf, -inf):
                refuse(E_INVALID, (name, i, v), cfg=with_entry(name, i, v))
    for v in (nan, 0.0, -0.0, -1.0, -inf):
        refuse(E_INVALID, ("clip_r2", v), cfg=with_entry("clip_r2", None, v))
    r.lens(with_entry("clip_r2", None, inf), to, None, **outs)             # +inf is allowed
    r.lens(good, to, None, **outs)
    r.synchronize()
    assert everything() == before                                          # (the defaults' clip_r2 is +inf: the same call again)
    # a non-finite entry of `to`
    for k in ("eye", "U", "V", "W"):
        for v in (nan, inf):
            bad = abi.WarpCamera.from_buffer_copy(bytes(to))
            getattr(bad, k).y = v
            refuse(E_INVALID, ("to", k, v), to=bad)
    # null arguments
    lp = C.byref(r.launchParams)
    assert L.fovpt_lens(None, lp, C.byref(good), None, None, None, None) == E_INVALID
    assert L.fovpt_lens(r._ctx, None, C.byref(good), None, None, None, None) == E_INVALID
    assert L.fovpt_lens(r._ctx, lp, None, None, None, None, None) == E_INVALID
    col_, rgba_ = C.c_void_p(), C.c_void_p()
    assert L.fovpt_lens_buffers(r._ctx, None, C.byref(rgba_)) == E_INVALID and L.fovpt_lens_buffers(r._ctx, C.byref(col_), None) == E_INVALID
    assert everything() == before
    # a null input
    f = r.launchParams.frame
    keep = f.accum_buffer
    f.accum_buffer = None
    refuse(E_INVALID, "null accum_buffer")
    f.accum_buffer = keep
    # aliasing: an output that is the input or the other output
    own_c, own_p = r.lens_buffers()
    refuse(E_INVALID, "out_color is in_color", in_color=oc.data_ptr())
    refuse(E_INVALID, "out_color is accum", out_color=keep)
    refuse(E_INVALID, "out_rgba is in_color", in_color=op.data_ptr())
    refuse(E_INVALID, "out_rgba is out_color", out_rgba=oc.data_ptr())
    refuse(E_INVALID, "the own colour is the input", out_color=None, in_color=own_c)
    refuse(E_INVALID, "the own rgba is the input", out_rgba=None, in_color=own_p)
    refuse(E_INVALID, "out_color is the own rgba", out_rgba=None, out_color=own_p)
    # the frame: another size, then a singular rendered camera (only `to` looks at it), then a tile shard
    f.size.x -= 4
    with pytest.raises(lib.FovptError) as e:
        r.lens(good, to, None, **outs)
    f.size.x += 4                                            # (the downloads of everything() go by this size)
    assert e.value.code == E_NO_FRAME and everything() == before
    cam = r.launchParams.camera
    keep_w = (cam.W.x, cam.W.y, cam.W.z)
    cam.W.set((cam.U.x, cam.U.y, cam.U.z))                   # determinant 0
    r.render()
    refuse(E_INVALID, "a singular rendered camera")
    r.lens(good, None, None, **outs)                         # without `to` the camera is not looked at
    cam.W.set(keep_w)
    c = r.config
    c.world, c.rank = 2, 0
    r.config = c
    r.render()
    before = everything()
    refuse(E_INVALID, "world 2")
    refuse(E_INVALID, "world 2, no re-aim", to=None)
    c.world, c.rank = 1, 0
    r.config = c
    r.render()
    r.lens(good, to, None, **outs)                           # the valid call after them
    r.synchronize()
    assert everything() != before
    r.close()


# ---- 5. the C++ drop-in ----------------------------------------------------------------------------------------------------------------
def test_cpp_dropin_lens(oracle, tmp_path):
    """SampleRenderer::lens() / lensForFrame() / downloadLens() of include/SimplePathtracer.h: the same pixels as Python."""
    exe, out = build_dropin(tmp_path, "lens_gpu_test"), str(tmp_path / "lens_out.bin")
    run_dropin(exe, out)
    size = (160, 96)
    n = size[0] * size[1]
    raw = np.fromfile(out, np.uint8)
    px = raw[:8 * n].view(np.uint32).reshape(2, size[1], size[0])
    col = raw[8 * n:40 * n].view(np.float32).reshape(2, size[1], size[0], 4)
    fitted = abi.LensConfig.from_buffer_copy(raw[40 * n:40 * n + 128].tobytes())
    r = dropin_renderer()
    r.render()
    assert bytes(fitted) == bytes(renderer.SampleRenderer.lens_for_frame(renderer.SampleRenderer.lens_defaults(), *size))
    r.lens()
    got_c, got_p = r.downloadLens()
    assert np.array_equal(px[0], got_p) and np.array_equal(bits(col[0]), bits(got_c))
    lc, full = lcfg(size, filter=abi.LENS_BICUBIC, encode=abi.LENS_ENCODE_RESOLVE)
    to = renderer.Camera((4.0, 3.0, 6.0), (0.3, 0.5, -0.2), BOX_CAMERA["up"], BOX_CAMERA["fovy"], size[0] / float(size[1]))
    r.lens(lc, to)
    got_c, got_p = r.downloadLens()
    assert np.array_equal(px[1], got_p) and np.array_equal(bits(col[1]), bits(got_c))
    want = lr.lens(oracle, r.downloadAccum(), full, camera(r), camera_of_to(to))
    assert np.array_equal(bits(got_c), bits(want["color"])) and np.array_equal(got_p, want["rgba"])
    assert (px[1] != px[0]).mean() > 0.05 and len(np.unique(px[0])) > 20
    r.close()


def camera_of_to(camera):
    to = renderer.SampleRenderer.warp_camera(camera)
    vec = lambda q: (float(q.x), float(q.y), float(q.z))
    return dict(eye=vec(to.eye), U=vec(to.U), V=vec(to.V), W=vec(to.W))
