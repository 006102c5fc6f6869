"""fovpt_warp_motion on the GPU against tests/warp_motion_ref.py, bit for bit: a translated and then turned box under three camera
motions, three advances and three fill radii, after a refit and after a rebuild; equality with fovpt_warp where nothing may differ;
the caller's G-buffer and the host's check of the hit records that go with it; the geometry against the production traversal after
the next update; ordering with frames in flight; every rejection; the C++ drop-in.  The restatement is fed the GPU's own G-buffer,
hit records and inputs; the conditions that keep a case from being vacuous are asserted on the restatement's output."""
import ctypes as C

import numpy as np
import pytest

import transform_ref as tf
import warp_motion_ref as wm
import warp_ref as wr
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer

from common import cfg_foveated
from gpu_common import (BOX_CAMERA, bits, box_renderer, build_dropin, camera, debug_buffer, device_images, dropin_renderer,
                        host_view, run_dropin)
from test_temporal_gpu import _scene_again
from test_warp_gpu import MOTIONS, SIZE, counts_of, to_camera, wcfg
from warp_motion_common import Intervals, check, frame_data, mcfg

pytestmark = pytest.mark.gpu
E_INVALID, E_NO_SCENE, E_NO_FRAME = -1, -3, -5
BOX = 1                                                  # box_model(): mesh 0 is the slab, mesh 1 the red box
N = SIZE[0] * SIZE[1]


def shift(t):
    """The transform that carries the box's rest positions by t."""
    m = tf.IDENTITY.copy()
    m[:, 3] = t
    return m


def turned(model, deg, t):
    """The box's rest positions turned by deg about its own vertical axis and carried by t."""
    return tf.apply(model.meshes[BOX].vertex, tf.rotation_translation(deg, (0.0, 0.5, 0.0), t))


def next_frame(r, k):
    """Another gaze and sample set, the camera as it is."""
    r.launchParams.frame.c.x, r.launchParams.frame.c.y = SIZE[0] // 2 + 9 * k - 15, SIZE[1] // 2 + 5 * k - 7
    r.launchParams.frame.subframe_index = k
    r.render()


def on_box(ck, gb):
    p = gb["prim"]
    return (p != wr.MISS) & (ck.mesh_of_prim[np.where(p == wr.MISS, 0, p).astype(np.int64)] == BOX)


def warp_both(r, to, cfg_m, gbuffer=None):
    """fovpt_warp and fovpt_warp_motion of the same arguments -> two (colour, rgba, map, counts)."""
    out = []
    for motion in (False, True):
        oc, op, om = device_images(SIZE, 16, 4, 4)
        if motion:
            r.warp_motion(to, cfg_m, gbuffer, None, None, oc.data_ptr(), op.data_ptr(), om.data_ptr())
        else:
            r.warp(to, wcfg(images=cfg_m.images, fill_radius=cfg_m.fill_radius), gbuffer, None, None, oc.data_ptr(), op.data_ptr(), om.data_ptr())
        out.append((oc.cpu().numpy().tobytes(), op.cpu().numpy().tobytes(), om.cpu().numpy().tobytes(), counts_of(r)))
    return out


# ---- 1. bit for bit ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[False, True], ids=["refit", "rebuild"])
def moved_box(request):
    """render -> temporal_motion, the box carried through update_transforms, render -> temporal_motion, the box turned through
    update_vertices (a refit, or FOVPT_UPDATE_REBUILD: the record order changes, the primitive ids do not), render ->
    temporal_motion: the frame the warps below re-aim, with the GPU's own G-buffer, hit records and images."""
    r = box_renderer(SIZE, cfg_foveated(12, 36, (1, 1, 2)), write_guides=True)
    ck = Intervals(r)
    next_frame(r, 0)
    ck.end_interval()
    ck.update({BOX: shift((0.5, 0.0, -0.25))}, kind="transforms")
    next_frame(r, 1)
    ck.end_interval()
    ck.update({BOX: turned(r.model, 25.0, (1.0, 0.125, -0.75))}, rebuild=request.param)
    next_frame(r, 2)
    ck.end_interval()
    gb, uv = frame_data(r)
    state = dict(r=r, ck=ck, gb=gb, uv=uv, color=r.downloadAccum(), rgba=r.downloadPixels())
    yield state
    r.close()


@pytest.mark.parametrize("motion", ["identity", "slide", "turn"])
def test_bit_for_bit(moved_box, motion):
    s = moved_box
    r, ck, gb, uv = s["r"], s["ck"], s["gb"], s["uv"]
    assert ck.moved_last() and ck.last["moved"].tolist() == [False, True]
    assert on_box(ck, gb).sum() >= 100                       # source pixels on the moved mesh
    to, want_cam = to_camera(motion)
    for advance in (0.5, 1.0, 2.5):
        for radius in (0, 2, 4):
            images = wr.RGBA if (advance, radius) == (1.0, 2) else wr.COLOR if (advance, radius) == (2.5, 0) else 3
            want = check(r, ck, to, want_cam, gb, uv, s["color"], s["rgba"], advance, radius, images, label=(motion, advance, radius))
            plain = wr.warp(gb, camera(r), want_cam, dict(images=images, fill_radius=radius), s["color"], s["rgba"])
            assert (want["map"] != plain["map"]).sum() > 50, (motion, advance, radius)
            assert (wr.collisions(want["dest"]) >= 2).any(), (motion, advance, radius)
            if radius:
                assert want["counts"][2] > 0, (motion, advance, radius)
            else:
                assert want["counts"][2] == 0
    # the frame is as it was
    assert np.array_equal(bits(r.downloadAccum()), bits(s["color"])) and np.array_equal(r.downloadPixels(), s["rgba"])


def test_the_renderers_own_buffers_serve_both_warps(moved_box):
    s = moved_box
    r, ck = s["r"], s["ck"]
    to, want_cam = to_camera("slide")
    want = wm.warp(s["gb"], s["uv"], ck.last, camera(r), want_cam, None, s["color"], s["rgba"])
    r.warp_motion(to)
    assert np.array_equal(bits(r.downloadWarpedColor()), bits(want["color"])) and np.array_equal(r.downloadWarpedPixels(), want["rgba"])
    assert counts_of(r) == want["counts"]
    p, nbytes = debug_buffer(r, "warp_keys")
    assert np.array_equal(r.download(p, np.empty((SIZE[1], SIZE[0]), np.uint64)), want["keys"])
    plain = wr.warp(s["gb"], camera(r), want_cam, None, s["color"], s["rgba"])
    r.warp(to)
    assert np.array_equal(r.downloadWarpedPixels(), plain["rgba"]) and counts_of(r) == plain["counts"] != want["counts"]


# ---- 2. it is fovpt_warp where it must be --------------------------------------------------------------------------------------------
def test_it_is_fovpt_warp_where_it_must_be():
    to, _ = to_camera("slide")
    r = box_renderer(SIZE, cfg_foveated(12, 36, (1, 1, 2)), write_guides=True)
    ck = Intervals(r)
    # (d) the first frame: update -> render -> the first temporal_motion.  Tracking starts there: the step had no history
    ck.update({BOX: shift((0.5, 0.0, 0.0))}, kind="transforms")
    next_frame(r, 0)
    ck.end_interval()
    assert ck.last is None
    for advance in (1.0, 4.0):
        a, b = warp_both(r, to, mcfg(advance=advance))
        assert a == b, ("first frame", advance)
    # (b) advance 0 with a moved box, and (the test is not vacuous) any other advance differs
    ck.update({BOX: shift((1.0, 0.0, 0.0))}, kind="transforms")
    next_frame(r, 1)
    ck.end_interval()
    assert ck.moved_last()
    a, b = warp_both(r, to, mcfg(advance=0.0))
    assert a == b, "advance 0"
    a, b = warp_both(r, to, mcfg(advance=1.0))
    assert a[2] != b[2] and a[3] != b[3]
    # (c) the box moved in the interval before the last one and not in the last
    next_frame(r, 2)
    ck.end_interval()
    assert ck.last is not None and not ck.moved_last()
    for advance in (0.5, 1.0, 4.0):
        a, b = warp_both(r, to, mcfg(advance=advance, fill_radius=4))
        assert a == b, ("moved before", advance)
    # a plain fovpt_temporal step ends an interval too
    ck.update({BOX: shift((1.5, 0.0, 0.0))}, kind="transforms")
    next_frame(r, 3)
    ck.end_interval("temporal")
    a, b = warp_both(r, to, mcfg(advance=1.0))
    assert a[2] != b[2]
    # (a) no update in the last interval, through every kind of step and G-buffer
    for k, how in enumerate(("temporal", "temporal_motion", "post")):
        next_frame(r, 4 + k)
        ck.end_interval(how)
        for gbuffer in (None, r.temporal_gbuffer()):
            a, b = warp_both(r, to, mcfg(advance=2.0), gbuffer)
            assert a == b, ("no update", how)
    r.close()


# ---- 3. the caller's G-buffer --------------------------------------------------------------------------------------------------------
def test_the_callers_gbuffer_and_the_hit_records_that_go_with_it():
    r = box_renderer(SIZE, cfg_foveated(12, 36, (1, 1, 2)), write_guides=True)
    ck = Intervals(r)
    to, want_cam = to_camera("turn")
    for k, t in enumerate(((0.0, 0.0, 0.0), (0.5, 0.0, 0.25))):
        ck.update({BOX: shift(t)}, kind="transforms")
        next_frame(r, k)
        ck.end_interval("post")
    g = r.temporal_gbuffer()
    cfg = mcfg(advance=1.5)

    def run(gbuffer):
        oc, op, om = device_images(SIZE, 16, 4, 4)
        r.warp_motion(to, cfg, gbuffer, None, None, oc.data_ptr(), op.data_ptr(), om.data_ptr())
        return host_view(oc, "color").tobytes(), host_view(op, "rgba").tobytes(), host_view(om, "map"), counts_of(r)

    def refused(gbuffer, label):
        with pytest.raises(lib.FovptError) as e:
            r.warp_motion(to, cfg, gbuffer)
        assert e.value.code == E_NO_FRAME, label

    with_g = run(g)                                          # the post step's trace: its set and the hit records it left
    own = run(None)
    assert with_g[:2] == own[:2] and np.array_equal(with_g[2], own[2]) and with_g[3] == own[3]
    gb, uv = frame_data(r)                                   # a fovpt_gbuffer call of the same frame in between invalidates nothing
    assert run(g)[3] == own[3]
    want = wm.warp(gb, uv, ck.last, camera(r), want_cam, dict(advance=1.5), r.downloadAccum(), r.downloadPixels())
    assert np.array_equal(own[2], want["map"]) and own[3] == want["counts"]
    assert (want["map"] != wr.warp(gb, camera(r), want_cam, None, r.downloadAccum(), r.downloadPixels())["map"]).sum() > 50
    # another view's trace overwrites the hit records: refused until the frame's own is traced again
    aspect = SIZE[0] / float(SIZE[1])
    r.setCamera(renderer.Camera(*MOTIONS["turn"], BOX_CAMERA["up"], BOX_CAMERA["fovy"], aspect))
    r.gbuffer()
    r.setCamera(renderer.Camera(BOX_CAMERA["eye"], BOX_CAMERA["lookat"], BOX_CAMERA["up"], BOX_CAMERA["fovy"], aspect))
    refused(g, "another view's hit records")
    assert run(None)[3] == own[3]                            # the call's own trace refreshes them
    assert run(g)[3] == own[3]
    # a further frame: the step's G-buffer and the hit records are the previous frame's
    r.render_async()
    refused(g, "a further render_async")
    r.synchronize()
    # an update issued since the step: refused with both kinds of G-buffer
    ck.update({BOX: shift((1.0, 0.0, 0.5))}, kind="transforms")
    refused(g, "an update since the step, the step's G-buffer")
    refused(None, "an update since the step, its own trace")
    r.gbuffer()
    refused(g, "an update since the step, traced again")
    next_frame(r, 3)
    refused(None, "rendered, not stepped")
    ck.end_interval("post")
    assert run(r.temporal_gbuffer())[3] == run(None)[3]
    r.close()


# ---- 4. the geometry, independent of the restatement ---------------------------------------------------------------------------------
def test_extrapolated_pixels_show_where_the_box_will_be():
    """The box moves by exactly (0.5, 0, 0) per step.  After fovpt_warp_motion(advance 1) and fovpt_warp to the same camera the
    next update is applied and fovpt_gbuffer traces the scene at that camera: over the direct pixels whose source is on the box,
    the source's primitive is the traced one more often for fovpt_warp_motion than for fovpt_warp."""
    r = box_renderer(SIZE, cfg_foveated(12, 36, (1, 1, 2)), write_guides=True)
    ck = Intervals(r)
    next_frame(r, 0)
    ck.end_interval()
    ck.update({BOX: shift((0.5, 0.0, 0.0))}, kind="transforms")
    next_frame(r, 1)
    ck.end_interval()
    to, _ = to_camera("slide")
    maps = []
    for motion in (True, False):
        om = device_images(SIZE, 16, 4, 4)[2]
        if motion:
            r.warp_motion(to, mcfg(images=abi.WARP_RGBA, advance=1.0), None, None, None, None, None, om.data_ptr())
        else:
            r.warp(to, wcfg(images=abi.WARP_RGBA), None, None, None, None, None, om.data_ptr())
        maps.append(host_view(om, "map").reshape(-1))
    gb = r.downloadGBuffer()
    rendered, box = gb["prim"].reshape(-1), on_box(ck, gb).reshape(-1)
    ck.update({BOX: shift((1.0, 0.0, 0.0))}, kind="transforms")      # the next update: where advance 1 says the box will be
    r.setCamera(renderer.Camera(*MOTIONS["slide"], BOX_CAMERA["up"], BOX_CAMERA["fovy"], SIZE[0] / float(SIZE[1])))
    target = r.downloadGBuffer()["prim"].reshape(-1)
    shares = []
    for m in maps:
        src, cls = m & np.uint32(0x3fffffff), m >> np.uint32(30)
        sel = (cls == abi.WARP_DIRECT) & box[src]
        assert sel.sum() >= 100
        shares.append(float((rendered[src][sel] == target[sel]).mean()))
    print("geometry: prim agrees with the trace after the next update: fovpt_warp_motion %.4f, fovpt_warp %.4f" % tuple(shares))
    assert shares[0] > shares[1]
    r.close()


# ---- 5. ordering ---------------------------------------------------------------------------------------------------------------------
def test_warp_motion_is_ordered_with_frames_in_flight():
    """update, render_async, post, warp_motion three times with no synchronisation in between: what the same sequence gives with a
    synchronise after every call."""
    import torch
    size = (384, 216)
    cfg = cfg_foveated(20, 60, (4, 8, 16))
    cfg.frames_in_flight = 2
    r = box_renderer(size, cfg, write_guides=True)
    to, _ = to_camera("slide", size)
    views = [((120, 90), 0), ((300, 40), 1), ((30, 200), 2)]
    moves = [shift((0.4 * (k + 1), 0.0, -0.2 * (k + 1))) for k in range(3)]
    outs = [[device_images(size, 16, 4, 4) for _ in views] for _ in range(2)]
    counts = []

    def frame(g, k):
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = g
        r.launchParams.frame.subframe_index = k

    for sync, out in zip((True, False), outs):
        # the box where it started with tracking on, the accum buffer's leftovers as all views leave them, no history
        r.update_transforms({BOX: shift((0.0, 0.0, 0.0))})
        for g, k in views:
            frame(g, k)
            r.render()
        r.post()
        r.temporal_reset()
        for (g, k), (oc, op, om) in zip(views, out):
            r.update_transforms({BOX: moves[k]})
            if sync:
                r.synchronize()
            frame(g, k)
            r.render_async()
            if sync:
                r.synchronize()
            r.post()
            if sync:
                r.synchronize()
            r.warp_motion(to, mcfg(advance=1.0), r.temporal_gbuffer() if k == 1 else None, None, None, oc.data_ptr(), op.data_ptr(), om.data_ptr())
            if sync:
                r.synchronize()
        r.synchronize()
        counts.append(counts_of(r))
    for want, got in zip(*outs):
        for x, y in zip(want, got):
            assert torch.equal(x, y)
    assert counts[0] == counts[1]
    # the last frame's extrapolation is not fovpt_warp's: the comparison is of moved pixels
    om = device_images(size, 16, 4, 4)[2]
    r.warp(to, None, None, None, None, None, None, om.data_ptr())
    assert (host_view(om, "map") != host_view(outs[1][2][2], "map")).sum() > 100
    r.close()


# ---- 6. rejections -------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_everything_unchanged():
    a, b = (box_renderer(SIZE, cfg_foveated(12, 36, (1, 1, 2)), write_guides=True) for _ in range(2))                        # a: the twin that is never refused
    to, _ = to_camera("slide")
    L = lib.load()
    outs = device_images(SIZE, 16, 4, 4)
    oc, op, om = outs
    ptrs = dict(out_color=oc.data_ptr(), out_rgba=op.data_ptr(), out_map=om.data_ptr())

    def refuse(code, label, **kw):
        args = dict(to=to, cfg=None, gbuffer=None, in_color=None, in_rgba=None, **ptrs)
        args.update(kw)
        with pytest.raises(lib.FovptError) as e:
            b.warp_motion(**args)
        assert e.value.code == code, label

    def both(fn):
        for r in (a, b):
            fn(r)

    refuse(E_NO_FRAME, "nothing rendered")
    both(lambda r: next_frame(r, 0))
    refuse(E_NO_FRAME, "no temporal step yet")
    both(lambda r: r.temporal())
    refuse(E_NO_FRAME, "only plain fovpt_temporal steps so far")
    refuse(E_NO_FRAME, "only plain steps, the step's G-buffer", gbuffer=b.temporal_gbuffer())
    assert counts_of(b) == (0, 0, 0, 0)
    with pytest.raises(lib.FovptError):                      # nothing was allocated
        debug_buffer(b, "warp_keys")
    for k in (1, 2):
        both(lambda r: r.update_transforms({BOX: shift((0.5 * k, 0.0, 0.0))}))
        both(lambda r: next_frame(r, k))
        both(lambda r: r.temporal_motion())
    b.warp_motion(to, None, None, None, None, **ptrs)
    b.warp_motion(to)
    g = b.temporal_gbuffer()
    b.gbuffer()
    b.synchronize()

    def everything():
        return (bytes(b.warp_counts()), b.downloadWarpedColor().tobytes(), b.downloadWarpedPixels().tobytes(), oc.cpu().numpy().tobytes(),
                op.cpu().numpy().tobytes(), om.cpu().numpy().tobytes(), b.download(debug_buffer(b, "warp_keys")[0], np.empty(N, np.uint64)).tobytes(),
                b.downloadAccum().tobytes(), b.downloadPixels().tobytes(), b.downloadTemporalHistory().tobytes(), b.downloadTemporalColor().tobytes())

    before = everything()

    def refuse_unchanged(code, label, **kw):
        refuse(code, label, **kw)
        assert everything() == before, label

    # the new errors: advance and the reserved fields
    for v in (float("nan"), float("inf"), -float("inf"), -1e-7, -1.0, float(np.nextafter(np.float32(abi.WARP_MAX_ADVANCE), np.float32(5))), 1e30):
        refuse_unchanged(E_INVALID, ("advance", v), cfg=mcfg(advance=v))
    for i in range(5):
        c = mcfg()
        c._reserved[i] = 1
        refuse_unchanged(E_INVALID, ("_reserved", i), cfg=c)
    for v in (0.0, abi.WARP_MAX_ADVANCE):                    # the bounds themselves are accepted
        b.warp_motion(to, mcfg(advance=v), g)
    b.warp_motion(to, None, None, None, None, **ptrs)
    b.warp_motion(to)
    assert everything() == before                            # (the same two warps again)
    # fovpt_warp's errors through the new entry point
    for images in (0, 4, -1):
        refuse_unchanged(E_INVALID, ("images", images), cfg=mcfg(images=images))
    for radius in (-1, abi.WARP_MAX_RADIUS + 1):
        refuse_unchanged(E_INVALID, ("fill_radius", radius), cfg=mcfg(fill_radius=radius))
    bad = abi.WarpCamera.from_buffer_copy(bytes(to))
    bad.V.y = float("nan")
    refuse_unchanged(E_INVALID, "camera NaN", to=bad)
    flat = abi.WarpCamera.from_buffer_copy(bytes(to))
    flat.W = flat.U
    refuse_unchanged(E_INVALID, "singular", to=flat)
    good = mcfg()
    lp = C.byref(b.launchParams)
    assert L.fovpt_warp_motion(b._ctx, None, C.byref(to), C.byref(good), None, None, None, None, None, None) == E_INVALID
    assert L.fovpt_warp_motion(b._ctx, lp, None, C.byref(good), None, None, None, None, None, None) == E_INVALID
    assert L.fovpt_warp_motion(b._ctx, lp, C.byref(to), None, None, None, None, None, None, None) == E_INVALID
    for k, v in (("width", SIZE[0] - 1), ("prim", None)):
        wrong = abi.GBufferPtrs.from_buffer_copy(bytes(g))
        setattr(wrong, k, v)
        refuse_unchanged(E_INVALID, ("gbuffer", k), gbuffer=wrong)
    f = b.launchParams.frame
    keep = f.accum_buffer
    f.accum_buffer = None
    refuse(E_INVALID, "null accum_buffer")
    f.accum_buffer = keep                                    # (the downloads of everything() go by this pointer)
    assert everything() == before
    refuse_unchanged(E_INVALID, "out_color is in_color", in_color=oc.data_ptr())
    refuse_unchanged(E_INVALID, "out_map is out_rgba", out_map=op.data_ptr())
    refuse_unchanged(E_INVALID, "out_map is the keys", out_map=debug_buffer(b, "warp_keys")[0])
    refuse_unchanged(E_INVALID, "out_color is the G-buffer's position", gbuffer=g, out_color=g.position)
    f.size.x -= 4
    with pytest.raises(lib.FovptError) as e:
        b.warp_motion(to, **ptrs)
    f.size.x += 4
    assert e.value.code == E_NO_FRAME and everything() == before
    trav = b.launchParams.traversable
    b.launchParams.traversable = trav + 1                    # only the traced G-buffer needs the scene
    refuse_unchanged(E_NO_SCENE, "no scene")
    b.warp_motion(to, None, g, **ptrs)
    b.launchParams.traversable = trav
    assert everything() == before
    # the new errors: what the call asks of the last step and of the hit records
    both(lambda r: r.update_transforms({BOX: shift((1.5, 0.0, 0.0))}))
    refuse_unchanged(E_NO_FRAME, "an update since the step")
    refuse_unchanged(E_NO_FRAME, "an update since the step, the step's G-buffer", gbuffer=g)
    both(lambda r: next_frame(r, 3))
    both(lambda r: r.temporal_motion())
    b.temporal_reset()
    refuse(E_NO_FRAME, "fovpt_temporal_reset")
    a.temporal_reset()
    # the context that was refused goes on like its twin
    both(lambda r: next_frame(r, 4))
    both(lambda r: r.temporal_motion())
    for x, y in zip((a.downloadAccum(), a.downloadPixels(), a.downloadTemporalColor(), a.downloadTemporalHistory()),
                    (b.downloadAccum(), b.downloadPixels(), b.downloadTemporalColor(), b.downloadTemporalHistory())):
        assert np.array_equal(bits(x), bits(y))
    b.warp_motion(to, None, b.temporal_gbuffer(), **ptrs)    # the valid call after them
    assert counts_of(b)[1] > N // 2
    # after fovpt_set_scene, until the next motion step
    both(_scene_again)
    both(lambda r: next_frame(r, 5))
    refuse(E_NO_FRAME, "set_scene: no step")
    both(lambda r: r.temporal())
    refuse(E_NO_FRAME, "set_scene: tracking is off again")
    both(lambda r: next_frame(r, 6))
    both(lambda r: r.temporal_motion())
    b.warp_motion(to, None, b.temporal_gbuffer(), **ptrs)
    for x, y in zip((a.downloadAccum(), a.downloadTemporalHistory()), (b.downloadAccum(), b.downloadTemporalHistory())):
        assert np.array_equal(bits(x), bits(y))
    b.resize(SIZE)
    refuse(E_NO_FRAME, "fovpt_resize")
    for r in (a, b):
        r.close()


# ---- 7. the C++ drop-in --------------------------------------------------------------------------------------------------------------
def test_cpp_dropin_warp_motion(tmp_path):
    """SampleRenderer::warpMotion() / warpMotionExposed() of include/SimplePathtracer.h: the same pixels and counts as Python."""
    exe, out = build_dropin(tmp_path, "warp_motion_gpu_test"), str(tmp_path / "warp_motion_out.bin")
    run_dropin(exe, out)
    size = (160, 96)
    n = size[0] * size[1]
    raw = np.fromfile(out, np.uint32)
    px = raw[:4 * n].reshape(4, size[1], size[0])
    counts = raw[4 * n:].view(np.uint64).reshape(4, 4)
    r = dropin_renderer(write_guides=True)
    to, _ = to_camera(((3.5, 3.0, 6.5), (0.0, 0.5, 0.0)), size)
    r.render()
    r.post()
    r.update_transforms({BOX: shift((0.5, 0.0, -0.25))})
    r.render()
    r.post()
    r.expose(None, r.post_buffers()[0])
    ec, ep = r.expose_buffers()
    r.warp_motion(to, mcfg(advance=1.0), r.temporal_gbuffer(), ec, ep)
    assert np.array_equal(px[0], r.downloadWarpedPixels()) and np.array_equal(px[1], px[0])
    assert tuple(counts[0]) == counts_of(r) == tuple(counts[1])
    r.warp_motion(to, mcfg(images=abi.WARP_RGBA, fill_radius=0, advance=2.5))
    assert np.array_equal(px[2], r.downloadWarpedPixels()) and tuple(counts[2]) == counts_of(r)
    r.warp(to, None, None, ec, ep)
    assert np.array_equal(px[3], r.downloadWarpedPixels()) and tuple(counts[3]) == counts_of(r)
    assert (px[3] != px[0]).sum() > 50 and counts[2][2] == 0 and len(np.unique(px[0])) > 20
    r.close()
