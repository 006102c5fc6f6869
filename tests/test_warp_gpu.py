"""fovpt_warp on the GPU against tests/warp_ref.py, bit for bit: six camera motions with every fill radius and image choice, a
FOV_OFF frame, the atrium, the caller's G-buffer (fovpt_temporal_gbuffer) against the call's own trace, ordering with frames in
flight, the geometry against the production traversal at the new camera, every rejection, reallocation, and the C++ drop-in.
The restatement is fed the GPU's own G-buffer and inputs; the conditions that keep a case from being vacuous are asserted on the
restatement's output."""
import ctypes as C

import numpy as np
import pytest

import warp_ref as wr
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer, scenes

from common import cfg_foveated, cfg_uniform, make_gpu
from gpu_common import (BOX_CAMERA, bits, box_renderer, build_dropin, camera, debug_buffer, device_images, dropin_renderer,
                        host_view, run_dropin, upload, with_entries)

pytestmark = pytest.mark.gpu
E_INVALID, E_NO_SCENE, E_NO_FRAME = -1, -3, -5
SIZE = (193, 109)                                   # odd, and no multiple of the kernels' 64 x 4 tile: partial edge tiles
PROBE = scenes.ambient_probe(64, 32, 2.5)
# the box scene's camera is at (4, 3, 6) and looks at (0, 0.5, 0): eye, lookat of the camera to warp to
MOTIONS = dict(identity=((4.0, 3.0, 6.0), (0.0, 0.5, 0.0)),
               slide=((4.333, 3.0, 5.778), (0.333, 0.5, -0.222)),
               turn=((4.0, 3.0, 6.0), (1.2, 0.5, -1.0)),
               dolly_in=((3.2, 2.5, 4.8), (0.0, 0.5, 0.0)),
               dolly_out=((4.8, 3.5, 7.2), (0.0, 0.5, 0.0)),
               behind=((1.0, 1.0, 1.5), (0.0, 0.5, 0.0)))     # inside the scene: the slab at the frame's bottom is behind this camera


def to_camera(motion, size=SIZE, base=BOX_CAMERA):
    """-> (abi.WarpCamera, the dict the restatement takes) of MOTIONS[motion] (or an (eye, lookat) pair)."""
    eye, lookat = MOTIONS[motion] if isinstance(motion, str) else motion
    to = renderer.SampleRenderer.warp_camera(renderer.Camera(eye, lookat, base["up"], base["fovy"], size[0] / float(size[1])))
    vec = lambda v: (float(v.x), float(v.y), float(v.z))
    return to, dict(eye=vec(to.eye), U=vec(to.U), V=vec(to.V), W=vec(to.W))


def wcfg(**d):
    return with_entries(renderer.SampleRenderer.warp_defaults(), d)


def counts_of(r):
    n = r.warp_counts()
    return (n.splatted, n.direct, n.filled, n.empty)


def check(r, to, want_cam, gb, color, rgba, radius, images, in_ptrs=(None, None), gbuffer=None, label=None):
    """One warp into caller's buffers against the restatement: every pixel of every enabled output, the map and the four
    counts; an image that is not enabled keeps its bytes.  -> the restatement's output."""
    f = r.launchParams.frame
    size = (f.size.x, f.size.y)
    oc, op, om = device_images(size, 16, 4, 4)
    r.warp(to, wcfg(images=images, fill_radius=radius), gbuffer, in_ptrs[0], in_ptrs[1], oc.data_ptr(), op.data_ptr(), om.data_ptr())
    got_counts = counts_of(r)
    want = wr.warp(gb, camera(r), want_cam, dict(images=images, fill_radius=radius), color, rgba)
    assert np.array_equal(host_view(om, "map"), want["map"]), label
    assert got_counts == want["counts"] and sum(got_counts[1:]) == size[0] * size[1], (label, got_counts, want["counts"])
    if images & wr.COLOR:
        assert np.array_equal(bits(host_view(oc, "color")), bits(want["color"])), label
    else:
        assert (oc.cpu().numpy() == 0x5a).all(), label
    if images & wr.RGBA:
        assert np.array_equal(host_view(op, "rgba"), want["rgba"]), label
    else:
        assert (op.cpu().numpy() == 0x5a).all(), label
    return want


def non_vacuous(want, motion, n):
    """What the issue asks of a case, on the restatement's output."""
    splatted, direct, filled, empty = want["counts"]
    if motion == "identity":
        return
    assert (wr.collisions(want["dest"]) >= 2).any(), motion        # destination pixels with two or more landed sources
    if motion == "dolly_in":
        assert filled > 0 and 2 * direct > n, (motion, want["counts"])
    if motion == "turn":
        assert empty > 0, (motion, want["counts"])
    if motion == "behind":
        hit = want["depth"] != wr.MISS_DEPTH                       # (a hit's depth word is the bits of a.z)
        assert (hit & (want["depth"] >= 0x80000000)).sum() > 50, motion      # sources behind the camera: a.z < 0


# ---- 1. bit for bit ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rendered_box():
    """One rendered box frame, its G-buffer and images, shared by the motions (none of them changes it)."""
    r = box_renderer(SIZE, cfg_foveated(12, 36, (1, 1, 2)), write_guides=True)
    r.render()
    gb = r.downloadGBuffer()
    state = dict(r=r, gb=gb, color=r.downloadAccum(), rgba=r.downloadPixels())
    yield state
    r.close()


@pytest.mark.parametrize("motion", list(MOTIONS))
def test_bit_for_bit(rendered_box, motion):
    s = rendered_box
    r, gb = s["r"], s["gb"]
    n = SIZE[0] * SIZE[1]
    to, want_cam = to_camera(motion)
    rng = np.random.default_rng(sorted(MOTIONS).index(motion))
    noise_c = rng.uniform(0, 8, (SIZE[1], SIZE[0], 4)).astype(np.float32)
    noise_c.reshape(-1, 4)[rng.permutation(n)[:64]] = (np.nan, np.inf, -0.0, 1e-42)      # copied bit for bit, whatever they hold
    noise_p = rng.integers(0, 1 << 32, (SIZE[1], SIZE[0]), dtype=np.uint64).astype(np.uint32)
    dev_c, dev_p = upload(noise_c), upload(noise_p)
    for radius in (0, 2, 4):
        for images in (1, 2, 3):
            want = check(r, to, want_cam, gb, s["color"], s["rgba"], radius, images, label=(motion, radius, images, "frame"))
            check(r, to, want_cam, gb, noise_c, noise_p, radius, images, (dev_c.data_ptr(), dev_p.data_ptr()), label=(motion, radius, images, "caller's"))
        if radius == 0:
            assert want["counts"][2] == 0
    non_vacuous(want, motion, n)
    if motion == "identity":
        # into the renderer's own buffers: the inputs, bit for bit
        r.warp(to)
        assert np.array_equal(bits(r.downloadWarpedColor()), bits(s["color"])) and np.array_equal(r.downloadWarpedPixels(), s["rgba"])
        assert counts_of(r) == (n, n, 0, 0)
        assert np.array_equal(want["map"], np.arange(n, dtype=np.uint32).reshape(SIZE[1], SIZE[0]))
    # the frame and its G-buffer are as they were
    assert np.array_equal(bits(r.downloadAccum()), bits(s["color"])) and np.array_equal(r.downloadPixels(), s["rgba"])


def test_some_winner_is_not_its_pixels_lowest_index_candidate(rendered_box):
    """The depth test decides, not the arrival or index order: among the cases above there are pixels where the two differ."""
    s = rendered_box
    odd = {}
    for motion in MOTIONS:
        dest, depth = wr.landing(s["gb"], camera(s["r"]), to_camera(motion)[1])
        odd[motion] = int(wr.winner_is_not_lowest(dest, wr.scatter(dest, depth)).sum())
    assert odd["identity"] == 0 and sum(odd.values()) > 20, odd


def test_fov_off_160x90():
    size = (160, 90)
    r = box_renderer(size, cfg_uniform(2), write_guides=True)
    r.render()
    gb, color, rgba = r.downloadGBuffer(), r.downloadAccum(), r.downloadPixels()
    for motion, radius in (("slide", 2), ("dolly_in", 4)):
        to, want_cam = to_camera(motion, size)
        want = check(r, to, want_cam, gb, color, rgba, radius, 3, label=motion)
        non_vacuous(want, motion, size[0] * size[1])
    r.close()


def test_the_atrium():
    """A scene with depth complexity (columns in front of walls), and the keys themselves."""
    r = make_gpu(scenes.atrium(8000), PROBE, scenes.ATRIUM_CAMERA, SIZE, cfg_foveated(12, 36, (1, 1, 2)))
    r.render()
    gb, color, rgba = r.downloadGBuffer(), r.downloadAccum(), r.downloadPixels()
    eye, lookat = scenes.ATRIUM_CAMERA["eye"], scenes.ATRIUM_CAMERA["lookat"]
    to, want_cam = to_camera(((eye[0] + 60.0, eye[1] + 10.0, eye[2] + 120.0), (lookat[0], lookat[1], lookat[2] + 60.0)), SIZE, scenes.ATRIUM_CAMERA)
    want = check(r, to, want_cam, gb, color, rgba, 2, 3, label="atrium")
    splatted, direct, filled, empty = want["counts"]
    assert (wr.collisions(want["dest"]) >= 2).sum() > 100 and filled > 100 and wr.winner_is_not_lowest(want["dest"], want["keys"]).any()
    p, nbytes = debug_buffer(r, "warp_keys")
    assert nbytes == SIZE[0] * SIZE[1] * 8
    assert np.array_equal(r.download(p, np.empty((SIZE[1], SIZE[0]), np.uint64)), want["keys"])
    r.close()


# ---- 2. the caller's G-buffer --------------------------------------------------------------------------------------------------------
def test_the_temporal_steps_gbuffer_saves_the_trace():
    """render -> post -> temporal_gbuffer -> warp(gbuffer=that) is warp(gbuffer=None) bit for bit; the buffers fovpt_gbuffer handed
    out keep their contents, and the inputs, the temporal history and a later frame are those of a context that never warped."""
    a, b = (box_renderer(SIZE, cfg_foveated(12, 36, (1, 1, 2)), write_guides=True) for _ in range(2))
    to, want_cam = to_camera("slide")
    for r in (a, b):
        with pytest.raises(lib.FovptError) as e:             # no temporal step yet
            r.temporal_gbuffer()
        assert e.value.code == E_NO_FRAME
        r.render()
        r.post()
    g = b.temporal_gbuffer()
    assert (g.width, g.height) == SIZE and g.prim and g.position
    b.warp(to)                                               # its own trace: into fovpt_gbuffer's buffers
    own = b.downloadWarpedColor(), b.downloadWarpedPixels(), counts_of(b)
    # fovpt_gbuffer's buffers now hold another view's G-buffer: the warp with the step's set must not touch them
    b.setCamera(renderer.Camera(*MOTIONS["turn"], BOX_CAMERA["up"], BOX_CAMERA["fovy"], SIZE[0] / float(SIZE[1])))
    other = b.gbuffer()
    b.setCamera(renderer.Camera(BOX_CAMERA["eye"], BOX_CAMERA["lookat"], BOX_CAMERA["up"], BOX_CAMERA["fovy"], SIZE[0] / float(SIZE[1])))
    assert other.prim != g.prim and other.position != g.position
    before = b.downloadGBuffer(other)
    oc, op, om = device_images(SIZE, 16, 4, 4)
    b.warp(to, None, g, None, None, oc.data_ptr(), op.data_ptr(), om.data_ptr())
    assert np.array_equal(bits(host_view(oc, "color")), bits(own[0])) and np.array_equal(host_view(op, "rgba"), own[1]) and counts_of(b) == own[2]
    after = b.downloadGBuffer(other)
    for k in before:
        assert np.array_equal(bits(before[k]), bits(after[k])), k
    assert (before["prim"] != b.downloadGBuffer(g)["prim"]).mean() > 0.05      # (the two sets do hold different views)
    # against the restatement on the step's set
    gb = b.downloadGBuffer(g)
    want = wr.warp(gb, camera(b), want_cam, None, b.downloadAccum(), b.downloadPixels())
    assert np.array_equal(host_view(om, "map"), want["map"]) and np.array_equal(bits(own[0]), bits(want["color"]))
    # the context that warped goes on like the one that did not
    for x, y in zip((a.downloadAccum(), a.downloadPixels(), a.downloadPostColor(), a.downloadTemporalHistory()),
                    (b.downloadAccum(), b.downloadPixels(), b.downloadPostColor(), b.downloadTemporalHistory())):
        assert np.array_equal(bits(x), bits(y))
    for r in (a, b):
        r.launchParams.frame.c.x += 11
        r.launchParams.frame.subframe_index = 1
        r.render()
        r.post()
    b.warp(to, None, b.temporal_gbuffer())
    for x, y in zip((a.downloadAccum(), a.downloadPixels(), a.downloadPostColor(), a.downloadPostPixels(), a.downloadTemporalHistory()),
                    (b.downloadAccum(), b.downloadPixels(), b.downloadPostColor(), b.downloadPostPixels(), b.downloadTemporalHistory())):
        assert np.array_equal(bits(x), bits(y))
    assert b.temporal_gbuffer().prim != g.prim               # the sets take turns
    with pytest.raises(lib.FovptError):                      # and that context never made warp buffers
        debug_buffer(a, "warp_keys")
    b.temporal_reset()
    with pytest.raises(lib.FovptError) as e:
        b.temporal_gbuffer()
    assert e.value.code == E_NO_FRAME
    for r in (a, b):
        r.close()


def test_warp_is_ordered_with_frames_in_flight():
    """render_async, warp, render_async, warp with no synchronisation in between: what the same sequence gives with a synchronise
    after every call."""
    import torch
    size = (384, 216)
    cfg = cfg_foveated(20, 60, (4, 8, 16))
    cfg.frames_in_flight = 2
    r = box_renderer(size, cfg, write_guides=True)
    to, _ = to_camera("slide", size)
    views = [((120, 90), 0), ((300, 40), 1), ((30, 200), 2)]
    outs = [[device_images(size, 16, 4, 4) for _ in views] for _ in range(2)]
    counts = [[], []]
    for sync, out, cnt in zip((True, False), outs, counts):
        for g, k in views:                                   # the accum buffer's leftovers where no pass writes, as all views leave them
            r.launchParams.frame.c.x, r.launchParams.frame.c.y = g
            r.launchParams.frame.subframe_index = k
            r.render()
        for (g, k), (oc, op, om) in zip(views, out):
            r.launchParams.frame.c.x, r.launchParams.frame.c.y = g
            r.launchParams.frame.subframe_index = k
            r.render_async()
            if sync:
                r.synchronize()
            r.warp(to, None, None, None, None, oc.data_ptr(), op.data_ptr(), om.data_ptr())
            if sync:
                r.synchronize()
                cnt.append(counts_of(r))
        r.synchronize()
        if not sync:
            cnt.append(counts_of(r))
    for want, got in zip(*outs):
        for x, y in zip(want, got):
            assert torch.equal(x, y)
    assert counts[1][0] == counts[0][-1]
    a, b = host_view(outs[0][0][1], "rgba"), host_view(outs[0][2][1], "rgba")
    assert (a != b).mean() > 0.1                             # (the frames differ: the comparison is not of copies)
    r.close()


# ---- 3. the geometry, against the production traversal -------------------------------------------------------------------------------
@pytest.mark.parametrize("motion", ["slide", "turn", "dolly_in"])
def test_warped_pixels_show_what_the_new_camera_sees(motion):
    """Independent of the restatement: over the direct pixels whose source is a hit, the source's primitive is the one fovpt_gbuffer
    traces at the `to` camera more often than the unwarped frame's primitive at the same pixel is."""
    r = box_renderer(SIZE, cfg_foveated(12, 36, (1, 1, 2)), write_guides=True)
    r.render()
    to, _ = to_camera(motion)
    om = device_images(SIZE, 16, 4, 4)[2]
    r.warp(to, wcfg(images=abi.WARP_RGBA), None, None, None, None, None, om.data_ptr())
    m = host_view(om, "map").reshape(-1)
    rendered = r.downloadGBuffer()["prim"].reshape(-1)      # (traced at the rendered camera)
    r.setCamera(renderer.Camera(*MOTIONS[motion], BOX_CAMERA["up"], BOX_CAMERA["fovy"], SIZE[0] / float(SIZE[1])))
    target = r.downloadGBuffer()["prim"].reshape(-1)        # the production traversal at the `to` camera
    src, cls = m & np.uint32(0x3fffffff), m >> np.uint32(30)
    sel = (cls == abi.WARP_DIRECT) & (rendered[src] != wr.MISS)
    warped = float((rendered[src][sel] == target[sel]).mean())
    unwarped = float((rendered[sel] == target[sel]).mean())
    print("geometry %s: %d direct hit pixels, prim agrees warped %.4f, unwarped %.4f" % (motion, int(sel.sum()), warped, unwarped))
    assert sel.sum() > 2000 and warped > unwarped
    r.close()


# ---- 4. rejections -------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_everything_unchanged():
    import torch
    r = box_renderer(SIZE, cfg_foveated(12, 36, (1, 1, 2)), write_guides=True)
    to, _ = to_camera("slide")
    L = lib.load()
    with pytest.raises(lib.FovptError) as e:                 # nothing rendered yet
        r.warp(to)
    assert e.value.code == E_NO_FRAME and counts_of(r) == (0, 0, 0, 0)
    r.render()
    oc, op, om = device_images(SIZE, 16, 4, 4)
    r.warp(to, None, None, None, None, oc.data_ptr(), op.data_ptr(), om.data_ptr())
    r.warp(to)
    g = r.gbuffer()
    r.synchronize()
    n = SIZE[0] * SIZE[1]

    def everything():
        return (bytes(r.warp_counts()), r.downloadWarpedColor().tobytes(), r.downloadWarpedPixels().tobytes(), oc.cpu().numpy().tobytes(),
                op.cpu().numpy().tobytes(), om.cpu().numpy().tobytes())

    before = everything()
    outs = dict(out_color=oc.data_ptr(), out_rgba=op.data_ptr(), out_map=om.data_ptr())

    def refuse(code, label, **kw):
        args = dict(to=to, cfg=None, gbuffer=None, in_color=None, in_rgba=None, **outs)
        args.update(kw)
        with pytest.raises(lib.FovptError) as e:
            r.warp(**args)
        assert e.value.code == code, label
        assert everything() == before, label

    # the config
    for images in (0, 4, 7, -1):
        refuse(E_INVALID, ("images", images), cfg=wcfg(images=images))
    for radius in (-1, abi.WARP_MAX_RADIUS + 1, 1 << 20):
        refuse(E_INVALID, ("fill_radius", radius), cfg=wcfg(fill_radius=radius))
    for i in range(6):
        c = wcfg()
        c._reserved[i] = 1
        refuse(E_INVALID, ("_reserved", i), cfg=c)
    # the camera
    for k in ("eye", "U", "V", "W"):
        for v in (float("nan"), float("inf"), -float("inf")):
            bad = abi.WarpCamera.from_buffer_copy(bytes(to))
            getattr(bad, k).y = v
            refuse(E_INVALID, (k, v), to=bad)
    flat = abi.WarpCamera.from_buffer_copy(bytes(to))
    flat.W = flat.U                                          # determinant 0
    refuse(E_INVALID, "singular", to=flat)
    flat.W.set((0.0, 0.0, 0.0))
    refuse(E_INVALID, "singular, W = 0", to=flat)
    # (a determinant that is not finite needs a non-finite entry: three binary32 factors cannot overflow binary64)
    # null arguments
    good = wcfg()
    lp = C.byref(r.launchParams)
    assert L.fovpt_warp(r._ctx, None, C.byref(to), C.byref(good), None, None, None, None, None, None) == E_INVALID
    assert L.fovpt_warp(r._ctx, lp, None, C.byref(good), None, None, None, None, None, None) == E_INVALID
    assert L.fovpt_warp(r._ctx, lp, C.byref(to), None, None, None, None, None, None, None) == E_INVALID
    col_, rgba_ = C.c_void_p(), C.c_void_p()
    assert L.fovpt_warp_buffers(r._ctx, None, C.byref(rgba_)) == E_INVALID and L.fovpt_warp_buffers(r._ctx, C.byref(col_), None) == E_INVALID
    assert L.fovpt_warp_counts(r._ctx, None) == E_INVALID and L.fovpt_temporal_gbuffer(r._ctx, None) == E_INVALID
    assert everything() == before
    # the G-buffer
    for k, v in (("width", SIZE[0] - 1), ("height", SIZE[1] + 1), ("prim", None), ("position", None)):
        bad = abi.GBufferPtrs.from_buffer_copy(bytes(g))
        setattr(bad, k, v)
        refuse(E_INVALID, ("gbuffer", k), gbuffer=bad)
    # an enabled image with a null input
    f = r.launchParams.frame
    keep = f.accum_buffer, f.frame_buffer
    f.accum_buffer = None
    refuse(E_INVALID, "null accum_buffer")
    refuse(E_INVALID, "null accum_buffer, COLOR", cfg=wcfg(images=abi.WARP_COLOR))
    f.accum_buffer, f.frame_buffer = keep[0], None
    refuse(E_INVALID, "null frame_buffer")
    f.frame_buffer = keep[1]
    # aliasing: an output that is an input or another output
    wc_, wp_ = r.warp_buffers()
    refuse(E_INVALID, "out_color is in_color", in_color=oc.data_ptr())
    refuse(E_INVALID, "out_color is accum", out_color=keep[0])
    refuse(E_INVALID, "out_rgba is frame_buffer", out_rgba=keep[1])
    refuse(E_INVALID, "out_rgba is in_rgba", in_rgba=op.data_ptr())
    refuse(E_INVALID, "out_map is in_rgba", in_rgba=om.data_ptr())
    refuse(E_INVALID, "out_map is out_rgba", out_map=op.data_ptr())
    refuse(E_INVALID, "out_map is out_color", out_map=oc.data_ptr())
    refuse(E_INVALID, "out_rgba is out_color", out_rgba=oc.data_ptr())
    refuse(E_INVALID, "out_map is the own colour", out_color=None, out_map=wc_)
    refuse(E_INVALID, "out_map is the G-buffer's prim", gbuffer=g, out_map=g.prim)
    refuse(E_INVALID, "out_color is the G-buffer's position", gbuffer=g, out_color=g.position)
    refuse(E_INVALID, "out_color is the traced G-buffer's position", out_color=g.position)
    refuse(E_INVALID, "out_map is the keys", out_map=debug_buffer(r, "warp_keys")[0])
    # the frame: another size, then a tile shard
    f.size.x -= 4
    with pytest.raises(lib.FovptError) as e:
        r.warp(to, **outs)
    f.size.x += 4                                            # (the downloads of everything() go by this size)
    assert e.value.code == E_NO_FRAME and everything() == before
    keep_trav = r.launchParams.traversable
    r.launchParams.traversable = keep_trav + 1               # not the current scene: only the traced G-buffer needs it
    refuse(E_NO_SCENE, "no scene")
    r.warp(to, None, g, **outs)
    assert everything() == before                            # (the same warp again, with a caller's G-buffer)
    r.launchParams.traversable = keep_trav
    c = r.config
    c.world, c.rank = 2, 0
    r.config = c
    r.render()
    refuse(E_INVALID, "world 2")
    c.world, c.rank = 1, 0
    r.config = c
    r.render()
    r.warp(to, **outs)                                       # the valid call after them
    assert counts_of(r)[1] > n // 2
    del torch
    r.close()


# ---- 5. reallocation -----------------------------------------------------------------------------------------------------------------
def test_resize_reallocates_the_warps_buffers():
    small, large = (96, 64), (200, 120)
    r = box_renderer(small, cfg_foveated(12, 36, (1, 1, 2)), write_guides=True)
    with pytest.raises(lib.FovptError) as e:
        r.warp_buffers()
    assert e.value.code == E_NO_FRAME
    with pytest.raises(lib.FovptError):
        debug_buffer(r, "warp_keys")
    r.render()
    r.warp(to_camera("slide", small)[0])
    assert debug_buffer(r, "warp_keys")[1] == small[0] * small[1] * 8
    r.resize(large)
    r.setCamera(r.lastSetCamera)
    r.launchParams.frame.c.x, r.launchParams.frame.c.y = 100, 60
    assert debug_buffer(r, "warp_keys")[1] == large[0] * large[1] * 8      # reallocated by the resize
    with pytest.raises(lib.FovptError) as e:                 # nothing rendered at this size yet
        r.warp(to_camera("slide", large)[0])
    assert e.value.code == E_NO_FRAME
    r.render()
    gb, color, rgba = r.downloadGBuffer(), r.downloadAccum(), r.downloadPixels()
    to, want_cam = to_camera("dolly_out", large)
    want = check(r, to, want_cam, gb, color, rgba, 2, 3, label="after resize")
    r.warp(to)
    assert np.array_equal(bits(r.downloadWarpedColor()), bits(want["color"])) and np.array_equal(r.downloadWarpedPixels(), want["rgba"])
    r.close()


# ---- 6. the C++ drop-in --------------------------------------------------------------------------------------------------------------
def test_cpp_dropin_warp(tmp_path):
    """SampleRenderer::warp() / warpExposed() / warpCounts() of include/SimplePathtracer.h: the same pixels and counts as Python."""
    exe, out = build_dropin(tmp_path, "warp_gpu_test"), str(tmp_path / "warp_out.bin")
    run_dropin(exe, out)
    size = (160, 96)
    n = size[0] * size[1]
    raw = np.fromfile(out, np.uint32)
    px = raw[:3 * n].reshape(3, size[1], size[0])
    counts = raw[3 * n:].view(np.uint64).reshape(3, 4)
    r = dropin_renderer(write_guides=True)
    to, _ = to_camera(((3.5, 3.0, 6.5), (0.0, 0.5, 0.0)), size)
    r.render()
    r.post()
    r.expose(None, r.post_buffers()[0])
    ec, ep = r.expose_buffers()
    r.warp(to, None, r.temporal_gbuffer(), ec, ep)
    assert np.array_equal(px[0], r.downloadWarpedPixels()) and np.array_equal(px[1], px[0])
    assert tuple(counts[0]) == counts_of(r) == tuple(counts[1])
    r.warp(to, wcfg(images=abi.WARP_RGBA, fill_radius=0))
    assert np.array_equal(px[2], r.downloadWarpedPixels()) and tuple(counts[2]) == counts_of(r)
    assert counts[2][2] == 0 and counts[0][2] > 0 and len(np.unique(px[0])) > 20
    r.close()
