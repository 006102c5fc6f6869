"""fovpt_temporal_motion on the GPU: identical to fovpt_temporal where nothing moves, bit for bit against
tests/temporal_motion_ref.py on the GPU's own inputs while meshes move (refit and rebuild, host and device pointers, two updates
between steps, a fovpt_temporal step in between, with and without motion vectors), an independent binary64 check of where a
turned block's pixels take their history from, the tracking rules, ordering with frames in flight, error codes and the C++
drop-in."""
import ctypes as C

import numpy as np
import pytest

import temporal_ref as tr
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer, scenes

from common import cfg_foveated, make_gpu
from gpu_common import bits, build_dropin, camera, debug_buffer, dropin_renderer, run_dropin
from temporal_common import tcfg
from temporal_motion_common import MotionChecker, download_hits, ramp_selection, vertex_arrays
from test_refit_gpu import cornell_motions, jitter, rotate_translate
from test_temporal_gpu import ALL_CAPS, _atrium, _scene_again, _view

pytestmark = pytest.mark.gpu
E_INVALID, E_NO_SCENE, E_NO_FRAME = -1, -3, -5
CORNELL = scenes.CORNELL_CAMERA
PROBE = scenes.ambient_probe(64, 32, 2.0)


def _cornell(size, cfg):
    cfg.write_guides = 1
    return make_gpu(scenes.cornell_box(), PROBE, CORNELL, size, cfg)


def _cornell_view(r, k, size):
    eye = (CORNELL["eye"][0] + 12.0 * k, CORNELL["eye"][1] + 6.0 * k, CORNELL["eye"][2] + 10.0 * k)
    r.setCamera(renderer.Camera(eye, CORNELL["lookat"], CORNELL["up"], CORNELL["fovy"], size[0] / float(size[1])))


# ---- 1. equivalence --------------------------------------------------------------------------------------------------------------
def test_without_updates_it_is_fovpt_temporal():
    size = (193, 109)
    a, b = (_atrium(size, cfg_foveated(15, 48, (1, 2, 8))) for _ in range(2))
    d = tcfg(ALL_CAPS)
    for k in range(6):
        for r in (a, b):
            _view(r, k, size)
            r.launchParams.frame.c.x, r.launchParams.frame.c.y = size[0] // 2 + 7 * k - 20, size[1] // 2 + 3 * k - 9
            r.render()
        a.temporal(d)
        b.temporal_motion(d)
        assert np.array_equal(bits(a.downloadTemporalColor()), bits(b.downloadTemporalColor())), k
        assert np.array_equal(a.downloadTemporalPixels(), b.downloadTemporalPixels()), k
        assert np.array_equal(bits(a.downloadTemporalHistory()), bits(b.downloadTemporalHistory())), k
    assert (b.downloadTemporalHistory()[..., 3] > 1).mean() > 0.5
    a.close()
    b.close()


def test_updates_that_rewrite_the_same_positions(oracle):
    """Every mesh is marked moved, X' is geometrically X: the barycentric path carries the history."""
    size = (193, 109)
    r = _atrium(size, cfg_foveated(15, 48, (1, 2, 8)))
    ck = MotionChecker(oracle, r, ALL_CAPS)
    same = {k: m.vertex for k, m in enumerate(r.model.meshes)}
    for k in range(6):
        _view(r, k, size)
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = size[0] // 2 + 7 * k - 20, size[1] // 2 + 3 * k - 9
        ck.update(same, device=bool(k & 1))
        r.render()
        _, h, _, _ = ck.step(with_motion=bool(k & 2))
    assert (h[..., 3] > 1).mean() > 0.5
    r.close()


# ---- 2. the restatement under motion -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [None, ALL_CAPS], ids=["defaults", "all_caps"])
def test_temporal_motion_matches_the_restatement(oracle, d):
    size = (192, 120)
    r = _cornell(size, cfg_foveated(12, 36, (1, 2, 4)))
    ck = MotionChecker(oracle, r, d)
    base = r.model
    (_, rigid), (_, scale), (_, point) = cornell_motions(base)
    tall, wall = base.meshes[4].vertex, base.meshes[2].vertex
    half = {4: rotate_translate(tall, 11.0, (368.0, 0.0, 351.0), (-20.0, 6.0, -15.0))}
    mesh = lambda gb: np.where(gb["prim"] == tr.MISS, -1, ck.mesh_of_prim[np.where(gb["prim"] == tr.MISS, 0, gb["prim"]).astype(np.int64)])

    def frame(k):
        _cornell_view(r, k, size)
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = size[0] // 2 + 9 * k - 20, size[1] // 2 + 4 * k - 8
        r.render()

    frame(0)
    ck.step()
    ck.update(rigid)                                          # host arrays, refit
    frame(1)
    _, h, cap, _ = ck.step(with_motion=False)                  # out_motion NULL
    on_tall = (mesh(ck.prev["gb"]) == 4) & (cap > 1)
    assert on_tall.sum() > 100 and (h[on_tall][:, 3] > 1).any()
    ck.update(scale, device=True)                             # device pointers, refit
    frame(2)
    ck.step(plain=True)                                       # fovpt_temporal in the middle: it ends the interval too
    ck.update(point, rebuild=True)                            # host arrays, FOVPT_UPDATE_REBUILD: the wall collapses to a point
    frame(3)
    ck.step()
    ck.update({2: wall, 4: half[4]})                          # two updates of one mesh between steps: the previous positions are
    ck.update({4: tall}, rebuild=True, device=True)           # those before the first; device pointers with a rebuild
    frame(4)
    _, h, cap, _ = ck.step()
    on_wall = (mesh(ck.prev["gb"]) == 2) & (cap > 1)            # the wall is back: its previous triangles have no area
    assert on_wall.sum() > 100 and (h[on_wall][:, 3] == 1).all()
    ck.update({3: base.meshes[3].vertex, 4: rigid[4]}, device=True)
    frame(5)
    _, h, _, mv = ck.step()
    assert (h[..., 3] > 1).mean() > 0.3 and (mv[..., 3] == 1).mean() > 0.5
    r.close()


# ---- 3. the ramp: where a turned block's pixels take their history from, in binary64 --------------------------------------------
def test_a_turned_block_takes_its_history_from_where_it_was():
    """Step 1 stores the ramp (x / w, y / h, 0.25) as history; the tall block is turned 23 degrees and carried, the camera moves;
    step 2 over a black frame gives out = H / 2.  On the block's side faces, away from edges, 2 out.b is 0.25 (n = 2) and
    (2 out.r w, 2 out.g h) is the binary64 projection, into the previous camera, of the binary64 barycentric point over the
    previous vertices, within 0.01 px: binary32 coordinates of magnitude <= 1e3 carry <= 6e-5 absolute error, below 1e-3 px at this
    size and depth, and the tolerance leaves tenfold room.  fovpt_temporal on a twin context restarts those pixels (n = 1): the
    turn changes the normal by |dN|^2 = 2 - 2 cos 23 = 0.159 > normal_tolerance = 0.1."""
    import torch
    size = (192, 120)
    w, h = size
    d = tcfg(dict(history_fovea=2, history_middle=2, history_periphery=2, history_uniform=2))
    y, x = np.mgrid[0:h, 0:w]
    ramp_h = np.stack([x / np.float32(w), y / np.float32(h), np.full((h, w), 0.25), np.ones((h, w))], axis=-1).astype(np.float32)
    ramp, zero = torch.from_numpy(ramp_h).cuda(), torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rs = [_cornell(size, cfg_foveated(12, 36, (1, 2, 4))) for _ in range(2)]
    new = cornell_motions(rs[0].model)[0][1]
    tri_vidx, vtx_prev, mesh_of_prim, _ = vertex_arrays(rs[0].model)
    outs = []
    for r, motion in zip(rs, (True, False)):
        step = (lambda p, m=None: r.temporal_motion(d, p, None, None, m)) if motion else (lambda p, m=None: r.temporal(d, p))
        r.render()
        step(ramp.data_ptr())
        if motion:
            prev_cam, pg = camera(r), r.downloadGBuffer()
        r.update_vertices(new)
        _cornell_view(r, 1, size)
        r.render()
        step(zero.data_ptr(), r.motion_buffer() if motion else None)
        outs.append((r.downloadTemporalColor(), r.downloadTemporalHistory(), r.downloadMotion() if motion else None))
        if motion:
            gb = r.downloadGBuffer()
            uv = download_hits(r)[..., 1:3]
    (out, hist, mv), (out_t, hist_t, _) = outs
    sel, px, py = ramp_selection(gb, uv, pg, prev_cam, size, 4, tri_vidx, vtx_prev, mesh_of_prim)
    print("ramp: %d pixels checked" % sel.sum())
    assert sel.sum() >= 300
    assert (2.0 * out[sel][:, 2] == 0.25).all() and (hist[sel][:, 3] == 2).all()
    ex = np.abs(2.0 * out[sel][:, 0].astype(np.float64) * w - px[sel])
    ey = np.abs(2.0 * out[sel][:, 1].astype(np.float64) * h - py[sel])
    mx = np.abs(mv[sel][:, 0].astype(np.float64) + x[sel] - px[sel])
    my = np.abs(mv[sel][:, 1].astype(np.float64) + y[sel] - py[sel])
    print("ramp: largest error %.2e px of the history, %.2e px of the motion vectors" % (max(ex.max(), ey.max()), max(mx.max(), my.max())))
    assert ex.max() <= 0.01 and ey.max() <= 0.01
    assert (mv[sel][:, 3] == 1).all() and mx.max() <= 0.01 and my.max() <= 0.01
    assert (hist_t[sel][:, 3] == 1).all() and not out_t[sel][:, :3].any()        # the camera alone: refused, out = in = 0
    for r in rs:
        r.close()


# ---- 4. the tracking rules --------------------------------------------------------------------------------------------------------
def test_an_update_before_tracking_starts_drops_the_history(oracle):
    size = (96, 64)
    r = _cornell(size, cfg_foveated(10, 24, (1, 2, 4)))
    ck = MotionChecker(oracle, r, ALL_CAPS)
    r.render()
    ck.step(plain=True)
    ck.update(cornell_motions(r.model)[0][1])                 # tracking is off: where the block was is not recorded
    r.render()
    acc = r.downloadAccum()
    c, h, _, mv = ck.step()                                   # (the checker expects no history either)
    assert np.array_equal(bits(c), bits(acc)) and (h[..., 3] == 1).all() and not mv.any()
    r.render()
    _, h, _, _ = ck.step()                                    # from here on it is carried, and updates are tracked
    assert (h[..., 3] > 1).mean() > 0.5
    ck.update(cornell_motions(r.model)[1][1])
    r.render()
    _, h, _, _ = ck.step()
    assert (h[..., 3] > 1).mean() > 0.5
    # an update before a fovpt_temporal step is behind the next step's previous step: the history stays
    r2 = _cornell(size, cfg_foveated(10, 24, (1, 2, 4)))
    ck2 = MotionChecker(oracle, r2, ALL_CAPS)
    ck2.update(cornell_motions(r2.model)[0][1])
    r2.render()
    ck2.step(plain=True)
    r2.render()
    _, h, _, _ = ck2.step()
    assert (h[..., 3] > 1).mean() > 0.5
    for q in (r, r2):
        q.close()


def test_temporal_motion_reset_paths(oracle):
    size = (160, 96)
    r = _cornell(size, cfg_foveated(12, 36, (1, 2, 4)))
    ck = MotionChecker(oracle, r, ALL_CAPS)
    motions = cornell_motions(r.model)

    def fresh(label):
        r.render()
        acc = r.downloadAccum()
        c, h, _, mv = ck.step()
        assert np.array_equal(bits(c), bits(acc)), label
        assert (h[..., 3] == 1).all() and not mv.any(), label

    def carried(k):
        ck.update(motions[k][1])
        r.render()
        _, h, _, _ = ck.step()
        assert (h[..., 3] > 1).mean() > 0.5

    fresh("first")
    carried(0)
    r.temporal_reset()
    ck.reset()
    fresh("reset")
    carried(1)
    r.resize((144, 80))
    r.setCamera(renderer.Camera(CORNELL["eye"], CORNELL["lookat"], CORNELL["up"], CORNELL["fovy"], 144 / 80.0))
    ck.reset()
    fresh("resize")
    carried(2)
    _scene_again(r)                                           # the model's own positions again, tracking off until the next step
    ck = MotionChecker(oracle, r, ALL_CAPS)
    with pytest.raises(lib.FovptError) as e:
        debug_buffer(r, "scene_vertices_prev")
    assert e.value.code == E_INVALID
    fresh("set_scene")
    carried(0)
    assert debug_buffer(r, "scene_vertices_prev")[1] == ck.vtx.size * 4
    r.close()


def test_a_context_that_never_steps_with_motion_keeps_no_previous_positions():
    size = (96, 64)
    r = _cornell(size, cfg_foveated(10, 24, (1, 2, 4)))
    for k in range(2):
        r.update_vertices(cornell_motions(r.model)[k][1])
        r.render()
        r.temporal()
    assert debug_buffer(r, "scene_vertices")[1] > 0
    with pytest.raises(lib.FovptError) as e:
        debug_buffer(r, "scene_vertices_prev")
    assert e.value.code == E_INVALID
    r.close()


# ---- 5. ordering ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["frames_in_flight", "chains_per_frame"])
def test_updates_and_steps_are_ordered_with_frames_in_flight(mode):
    """Update, render and step issued back to back over four frames, no synchronisation in between, into caller buffers: what the
    same sequence gives with a synchronise after every call."""
    import torch
    size = (384, 216)
    cfg = cfg_foveated(20, 60, (4, 8, 16))               # >= 16384 sample slots: chains_per_frame = 2 does split the frame
    if mode == "frames_in_flight":
        cfg.frames_in_flight = 2
    else:
        cfg.chains_per_frame = 2
    r = _atrium(size, cfg)
    orig = {k: m.vertex for k, m in enumerate(r.model.meshes)}
    nm = len(orig)
    views = [((120 + 40 * k, 90 + 15 * k), k) for k in range(4)]
    moves = [{m: jitter(orig[m], 100 * k + m, 25.0) for m in range(nm) if (m + k) % 3 == 0} for k in range(4)]
    dev = [{m: torch.from_numpy(v).cuda() for m, v in mv.items()} for mv in moves]
    torch.cuda.synchronize()

    def setup(g, k):
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = g
        r.launchParams.frame.subframe_index = 0
        _view(r, k, size)

    def begin():
        # the meshes where they started, the accum buffer's leftovers where no pass writes as all four views leave them, no history
        r.update_vertices(orig)
        for g, k in views:
            setup(g, k)
            r.render()
        r.temporal_reset()

    d = tcfg(ALL_CAPS)
    outs = [[(torch.empty((size[1], size[0], 4), dtype=torch.float32, device="cuda"), torch.empty((size[1], size[0]), dtype=torch.int32, device="cuda"),
              torch.empty((size[1], size[0], 4), dtype=torch.float32, device="cuda")) for _ in views] for _ in range(2)]
    torch.cuda.synchronize()
    hists = []
    for sync, out in zip((True, False), outs):
        begin()
        for ((g, k), (oc, op, om)) in zip(views, out):
            r.update_vertices(dev[k] if k & 1 else moves[k])   # device pointers and host arrays in turn
            if sync:
                r.synchronize()
            setup(g, k)
            r.render_async()
            if sync:
                r.synchronize()
            r.temporal_motion(d, None, oc.data_ptr(), op.data_ptr(), om.data_ptr())
            if sync:
                r.synchronize()
        r.synchronize()
        hists.append(r.downloadTemporalHistory())
    for want, got in zip(*outs):
        for a, b in zip(want, got):
            assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
    assert np.array_equal(bits(hists[0]), bits(hists[1]))
    assert (hists[0][..., 3] > 1).mean() > 0.5 and (outs[0][-1][2].cpu().numpy()[..., 3] == 1).mean() > 0.5
    r.close()


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------
def test_temporal_motion_errors():
    cfg = cfg_foveated(15, 48, (1, 2, 8))
    r = _atrium((96, 64), cfg)
    with pytest.raises(lib.FovptError) as e:             # nothing rendered yet
        r.temporal_motion()
    assert e.value.code == E_NO_FRAME
    r.render()
    r.temporal_motion()
    M = abi.TEMPORAL_MAX_HISTORY
    caps = ("history_fovea", "history_middle", "history_periphery", "history_uniform")
    bad = tuple((k, v) for k in caps for v in (0, -1, M + 1)) + tuple(
        (k, v) for k in ("normal_tolerance", "depth_tolerance") for v in (-1e-7, float("nan"), float("inf"), -float("inf"))) + (
        ("normal_tolerance", float(np.nextafter(np.float32(4), np.float32(5)))), ("depth_tolerance", float(np.nextafter(np.float32(1), np.float32(2)))))
    for k, v in bad:
        with pytest.raises(lib.FovptError) as e:
            r.temporal_motion(tcfg({k: v}))
        assert e.value.code == E_INVALID, (k, v)
    for d in (dict(zip(caps, (1, 1, 1, 1)), normal_tolerance=0.0, depth_tolerance=0.0),   # the bounds themselves are accepted
              dict(zip(caps, (M, M, M, M)), normal_tolerance=4.0, depth_tolerance=1.0)):
        r.temporal_motion(tcfg(d))
    for i in range(2):
        c = tcfg(None)
        c._reserved[i] = 1
        with pytest.raises(lib.FovptError) as e:
            r.temporal_motion(c)
        assert e.value.code == E_INVALID
    col, rgba, hist = r.temporal_buffers()
    with pytest.raises(lib.FovptError) as e:             # writing the history it reads
        r.temporal_motion(None, None, hist, None)
    assert e.value.code == E_INVALID
    mo = r.motion_buffer()
    f = r.launchParams.frame
    other = r.reconstruct_buffers()[0]                   # (a float4 frame of the context's that no step uses)
    for args in ((None, None, mo, None, mo),             # the motion buffer is the output colour,
                 (None, mo, None, None, mo),             # the input,
                 (None, None, None, None, f.accum_buffer),   # the input when that is the accum buffer,
                 (None, None, None, None, hist),         # the history the step reads or the one it writes,
                 (None, None, None, None, col),          # the context's own output colour,
                 (None, None, other, mo, mo)):           # the rgba8 output
        with pytest.raises(lib.FovptError) as e:
            r.temporal_motion(*args)
        assert e.value.code == E_INVALID, args
    r.temporal_motion()
    other_hist = r.temporal_buffers()[2]
    assert other_hist != hist
    for h_ in (hist, other_hist):
        with pytest.raises(lib.FovptError) as e:
            r.temporal_motion(None, None, None, None, h_)
        assert e.value.code == E_INVALID
    r.temporal_motion(None, None, None, None, mo)        # and a buffer of its own is accepted
    f.size.x -= 4
    with pytest.raises(lib.FovptError) as e:
        r.temporal_motion()
    assert e.value.code == E_NO_FRAME
    f.size.x += 4
    trav = r.launchParams.traversable
    r.launchParams.traversable = 12345
    with pytest.raises(lib.FovptError) as e:
        r.temporal_motion()
    assert e.value.code == E_NO_SCENE
    r.launchParams.traversable = trav
    L = lib.load()
    d = tcfg(None)
    assert L.fovpt_temporal_motion(r._ctx, None, C.byref(d), None, None, None, None) == E_INVALID
    assert L.fovpt_temporal_motion(r._ctx, C.byref(r.launchParams), None, None, None, None, None) == E_INVALID
    c = r.config
    c.world, c.rank = 2, 0
    r.config = c
    r.render()
    with pytest.raises(lib.FovptError) as e:             # a tile shard
        r.temporal_motion()
    assert e.value.code == E_INVALID
    r.close()


# ---- 8. the C++ drop-in -------------------------------------------------------------------------------------------------------------
def test_cpp_dropin_temporal_motion(tmp_path):
    """SampleRenderer::updateAccel() + temporalMotion() + downloadTemporalPixels / downloadMotion of include/SimplePathtracer.h:
    the same pixels and motion vectors as Python."""
    exe, out = build_dropin(tmp_path, "temporal_motion_gpu_test"), str(tmp_path / "temporal_motion_out.bin")
    run_dropin(exe, out)
    n = 160 * 96
    raw = np.fromfile(out, np.uint32)
    px = raw[:2 * n].reshape(2, 96, 160)
    mv = raw[2 * n:].view(np.float32).reshape(96, 160, 4)
    r = dropin_renderer(write_guides=True)
    model = r.model
    r.render()
    r.temporal_motion()
    assert np.array_equal(px[0], r.downloadTemporalPixels())
    r.update_vertices({1: (model.meshes[1].vertex + np.float32([0.5, 0.0, -0.25])).astype(np.float32)})
    r.render()
    r.temporal_motion(out_motion=r.motion_buffer())
    assert np.array_equal(px[1], r.downloadTemporalPixels())
    assert np.array_equal(bits(mv), bits(r.downloadMotion()))
    box = r.downloadGBuffer()["prim"]
    box = (box != tr.MISS) & (box >= len(model.meshes[0].index))
    assert box.sum() > 100 and (np.abs(mv[box][:, :2]).max(axis=-1) > 1).mean() > 0.5   # the box's pixels did move
    r.close()
