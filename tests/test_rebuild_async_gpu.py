"""FOVPT_UPDATE_REBUILD_ASYNC on the GPU: a hierarchy built beside the frames and swapped in.  No frame, accum buffer, G-buffer or
vertex depends on the flag or on when the new tree is adopted (bit for bit against a twin context without the flag, with frames in
flight and with two chains per frame); the adopted tree is a conservative tree of the present positions whose cost the builder
measured; the counters and the paths that end a build early; rejections; the temporal chain and the late warp across an
adoption; and the C++ drop-in.  FOVPT_ASYNC_BUILD_DELAY_MS holds the state at BUILDING where a test needs it there."""
import ctypes as C

import numpy as np
import pytest

import refit_ref as rf
import skin_ref as sk
import transform_ref as tf
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer, scenes

from common import cfg_foveated, make_gpu
from gpu_common import bits, build_dropin, dropin_renderer, run_dropin
from temporal_common import tcfg
from test_refit_gpu import hierarchy, jitter, moved, render
from test_rig_gpu import SHORT, TALL, morph_fixture
from test_transform_gpu import close, dbits, expected_cost, scene_vertices

pytestmark = pytest.mark.gpu
E_INVALID, E_NO_SCENE, E_NO_FRAME = -1, -3, -5
IDLE, BUILDING, READY = abi.REBUILD_IDLE, abi.REBUILD_BUILDING, abi.REBUILD_READY
CORNELL = scenes.CORNELL_CAMERA
PROBE = scenes.ambient_probe(64, 32, 2.0)
DELAY = "FOVPT_ASYNC_BUILD_DELAY_MS"
F = np.float32
CAPS = dict(history_fovea=3, history_middle=5, history_periphery=8, history_uniform=6)


# ---- helpers --------------------------------------------------------------------------------------------------------------
def animated_cornell(size, cfg):
    """The Cornell box with the tall block skinned and morphed, the short block morphed and the left wall on a rig node: every
    one of the five update calls has something to move."""
    base = scenes.cornell_box()
    skins, morphs, rig = morph_fixture(base)
    r = make_gpu(base, PROBE, CORNELL, size, cfg)
    r.set_skins(skins)
    r.set_morphs(morphs)
    r.set_rig(rig)
    return base, r


def cornell_updates(base):
    """Nine updates over all five entry points, as (method, argument tuple)."""
    tall, short = base.meshes[TALL].vertex, base.meshes[SHORT].vertex
    rng = np.random.default_rng(11)
    return [
        ("update_vertices", ({TALL: jitter(tall, 1, 6.0)},)),
        ("update_transforms", ({SHORT: tf.rotation_translation(20.0, (186.0, 0.0, 168.0), (15.0, 0.0, -10.0))},)),
        ("update_skinned", ({TALL: sk.bend_pose(tall, 3, 25.0, (-20.0, 0.0, 10.0))},)),
        ("update_morphed", ({SHORT: F([0.5, -0.25, 1.0])},)),
        ("update_animated", (0, 0.7)),
        ("update_vertices", ({SHORT: jitter(short, 2, 4.0), 2: jitter(base.meshes[2].vertex, 3, 3.0)},)),
        ("update_morphed", ({TALL: (rng.uniform(0.0, 1.0, 4).astype(F), sk.bend_pose(tall, 3, -15.0, (5.0, 0.0, 5.0)))},)),
        ("update_animated", (1, 0.5)),
        ("update_transforms", ({TALL: tf.rotation_translation(-30.0, (368.0, 0.0, 351.0), (-30.0, 0.0, -20.0))},)),
    ]


def call(r, update, rebuild=False):
    name, args = update
    getattr(r, name)(*args, rebuild=rebuild)


def new_frame(r, size):
    """A frame issued into buffers of its own, not synchronised."""
    import torch
    acc = torch.zeros((size[1], size[0], 4), dtype=torch.float32, device="cuda")
    px = torch.zeros((size[1], size[0]), dtype=torch.int32, device="cuda")
    f = r.launchParams.frame
    f.accum_buffer, f.frame_buffer = acc.data_ptr(), px.data_ptr()
    f.subframe_index = 0
    r.render_async()
    return acc, px


def host(frames):
    return [(a.cpu().numpy(), p.cpu().numpy()) for a, p in frames]


def same_frames(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(bits(g[0]), bits(w[0])) and np.array_equal(g[1], w[1]), "frame %d" % k


def gbuffer_bits(r):
    g = r.downloadGBuffer()
    return [g["prim"]] + [bits(g[k]) for k in ("position", "normal", "albedo")]


def split_vertices(model, vtx):
    out, first = {}, 0
    for k, m in enumerate(model.meshes):
        out[k] = vtx[first:first + m.vertex.shape[0]]
        first += m.vertex.shape[0]
    return out


def state(r, **kw):
    return r.rebuild_state(**kw)


def counters(info):
    return (info.requested, info.started, info.adopted, info.failed, info.discarded)


# ---- 1. frames do not depend on it ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["frames_in_flight", "chains_per_frame"])
def test_frames_do_not_depend_on_the_flag_or_the_swap(monkeypatch, mode):
    """Two contexts get the same nine updates over all five entry points, a frame after each and no synchronisation in between;
    one carries "async" on the second update and is held at BUILDING through the next six, is READY after a wait, adopts in the
    ninth update and renders four more frames.  Everything a frame can show is equal bit for bit, and the last frame is a fresh
    fovpt_set_scene's of the final positions."""
    import torch
    size = (192, 128)
    cfg = cfg_foveated(20, 48, (2, 4, 8))                   # >= 16384 sample slots: chains_per_frame = 2 does split the frame
    if mode == "frames_in_flight":
        cfg.frames_in_flight = 2
    else:
        cfg.chains_per_frame = 2
    cfg.write_guides = 1
    monkeypatch.setenv(DELAY, "600")
    results = {}
    for flagged in (False, True):                           # (the twin first: every kernel is loaded when the flagged run starts)
        base, r = animated_cornell(size, cfg)
        ups = cornell_updates(base)
        frames = []
        torch.cuda.synchronize()
        for k, u in enumerate(ups[:8]):
            call(r, u, "async" if flagged and k == 1 else False)
            frames.append(new_frame(r, size))
            if flagged and k >= 1:
                info = state(r)
                assert info.state == BUILDING, "update %d: the build has already ended (state %d)" % (k, info.state)
                assert counters(info) == (1, 1, 0, 0, 0) and info.snapshot_update == 2
        if flagged:
            assert state(r, wait=True).state == READY
            assert r.hierarchy_cost().updates == 8
        before = r.stats()
        call(r, ups[8])
        if flagged:
            info = state(r)
            assert info.state == IDLE and counters(info) == (1, 1, 1, 0, 0) and info.ms_build > 0
            assert r.hierarchy_cost().updates == 10         # the adoption counts as one more
            assert r.stats().ms_bvh_build != before.ms_bvh_build
        else:
            assert r.hierarchy_cost().updates == 9
        for _ in range(4):
            frames.append(new_frame(r, size))
        r.synchronize()
        f = r.launchParams.frame
        guides = [bits(r.download(getattr(f, name + "_buffer"), np.empty((size[1], size[0], 4), F))) for name in ("normal", "albedo", "color")]
        results[flagged] = (host(frames), gbuffer_bits(r), bits(scene_vertices(r)), guides)
        if flagged:
            final = split_vertices(base, scene_vertices(r))
        r.close()
    same_frames(results[True][0], results[False][0])
    for a, b in zip(results[True][1] + results[True][3], results[False][1] + results[False][3]):
        assert np.array_equal(a, b)
    assert np.array_equal(results[True][2], results[False][2])
    assert not np.array_equal(results[True][0][0][1], results[True][0][-1][1])
    fresh = make_gpu(moved(base, final), PROBE, CORNELL, size, cfg)
    acc, px, _ = render(fresh)
    last = results[True][0][-1]
    assert np.array_equal(bits(acc), bits(last[0])) and np.array_equal(px, last[1].view(np.uint32))
    fresh.close()


# ---- 2. the adopted tree ------------------------------------------------------------------------------------------------------
def atrium_case():
    model = scenes.atrium(8000)
    lo = np.min([m.vertex.min(axis=0) for m in model.meshes], axis=0)
    hi = np.max([m.vertex.max(axis=0) for m in model.meshes], axis=0)
    k = int(np.argmax([m.index.shape[0] for m in model.meshes]))
    carry = np.concatenate([np.eye(3), ((hi - lo) * 0.8).astype(np.float64)[:, None]], axis=1).astype(F)
    small = [("update_vertices", ({(k + 1) % len(model.meshes): jitter(model.meshes[(k + 1) % len(model.meshes)].vertex, 5, 10.0)},)),
             ("update_transforms", ({(k + 2) % len(model.meshes): tf.rotation_translation(4.0, (0.0, 0.0, 0.0), (3.0, 0.0, -2.0))},)),
             ("update_vertices", ({(k + 3) % len(model.meshes): jitter(model.meshes[(k + 3) % len(model.meshes)].vertex, 6, 10.0)},))]
    return model, k, carry, small


def test_the_adopted_tree_is_a_good_tree_of_the_present_positions(monkeypatch):
    """The atrium with its largest mesh carried 0.8 of the scene's extent: the refit tree's cost is above `built`.  The snapshot
    is taken there; two small updates follow while the build runs; the third adopts.

    How close the adopted tree comes to a synchronous rebuild is measured first: the same positions are built in fresh contexts.
    If their hierarchies are byte-identical the builder is deterministic and `built` must be bit-equal with a twin's that does
    FOVPT_UPDATE_REBUILD at the snapshot's positions (and `current`, after the same refits, too); if not, twice the measured
    relative spread of `built` is allowed.  A spread is measured no finer than the format resolves: two binary64 costs that
    differ at all differ by 2^-52 relative or more, so a measured spread of 0 stands for "below 2^-52" and counts as 2^-52.
    (Measured: the builds differ in the order of their nodes, which the build allocates with atomic counters, and so in the
    order of the cost's sum: `built` differs by one unit in the last place between some pairs of builds and by nothing between
    others, which is why four builds are measured and not two.)  Which case held is printed."""
    model, k, carry, small = atrium_case()
    monkeypatch.setenv(DELAY, "300")
    r = renderer.SampleRenderer(model)
    trav = r.launchParams.traversable
    c0 = r.hierarchy_cost()
    st0 = r.stats()
    r.update_transforms({k: carry}, rebuild="async")
    c1 = r.hierarchy_cost(wait=True)
    assert c1.current > c1.built and dbits(c1.built) == dbits(c0.built)          # the case is not vacuous
    for u in small[:2]:
        call(r, u)
        assert state(r).state == BUILDING
    info = state(r, wait=True)
    assert info.state == READY and info.snapshot_update == 1
    cb = r.hierarchy_cost(wait=True)
    assert cb.updates == 3 and info.snapshot_update < cb.updates                # the snapshot is older than the positions
    assert r.stats().ms_bvh_build == st0.ms_bvh_build                            # nothing is adopted outside the two places
    call(r, small[2])
    info = state(r)
    assert info.state == IDLE and info.adopted == 1 and info.failed == 0 and info.last_error == 0
    n, t = hierarchy(r)
    rf.check_conservative(n, t, rf.levels_of(n))
    ca = r.hierarchy_cost(wait=True)
    assert (ca.updates, ca.measured) == (5, 5)
    assert close(ca.current, expected_cost(r)), (ca.current, expected_cost(r))
    assert ca.current < cb.current and dbits(ca.built) != dbits(c0.built)
    st1 = r.stats()
    assert st1.ms_bvh_build != st0.ms_bvh_build and st1.ms_bvh_build == pytest.approx(info.ms_build, rel=1e-6)
    assert (st1.num_bvh_nodes * 128, st1.tri_bytes, st1.num_triangles) == (st1.bvh_bytes, t.shape[0] * 48, st0.num_triangles)
    assert n.shape[0] == st1.num_bvh_nodes
    assert r.launchParams.traversable == trav
    r.close()

    # `built` is the cost of the tree as built: a twin adopts through rebuild_state with no update in between
    monkeypatch.setenv(DELAY, "0")
    q = renderer.SampleRenderer(model)
    q.hierarchy_cost()
    q.update_transforms({k: carry}, rebuild="async")
    assert state(q, wait=True, adopt=True).adopted == 1
    cq = q.hierarchy_cost(wait=True)
    assert (cq.updates, cq.measured) == (2, 2)
    assert dbits(cq.current) == dbits(cq.built)                                  # the refit over the snapshot's positions changes no box
    assert close(cq.built, expected_cost(q)), (cq.built, expected_cost(q))
    for u in small:
        call(q, u)
    cq2 = q.hierarchy_cost(wait=True)
    q.close()

    # the builder's own spread: the snapshot's positions built in two fresh contexts
    at_snapshot = moved(model, tf.restate(model, {k: carry}))
    fresh = []
    for _ in range(4):
        s = renderer.SampleRenderer(at_snapshot)
        fresh.append((hierarchy(s), s.hierarchy_cost().built))
        s.close()
    identical = all(np.array_equal(a, b) for f in fresh[1:] for a, b in zip(fresh[0][0], f[0]))
    words = [max(int((a != b).sum()) if a.shape == b.shape else -1 for f in fresh[1:] for a, b in (((fresh[0][0][i], f[0][i]),))) for i in (0, 1)]
    costs = [f[1] for f in fresh]
    spread = (max(costs) - min(costs)) / min(costs)
    # the reference: a synchronous rebuild at the snapshot's positions, then the same refits
    w = renderer.SampleRenderer(model)
    w.hierarchy_cost()
    w.update_transforms({k: carry}, rebuild=True)
    for u in small:
        call(w, u)
    cw = w.hierarchy_cost(wait=True)
    w.close()
    rel_built, rel_current = abs(ca.built - cw.built) / cw.built, abs(ca.current - cw.current) / cw.current
    print("builder: hierarchies of four fresh builds %s (%d node words, %d record words), relative spread of built %.3g; async against synchronous rebuild: built %.17g / %.17g "
          "(rel %.3g), current %.17g / %.17g (rel %.3g); refit tree before adoption %.6g"
          % ("byte-identical" if identical else "differ", words[0], words[1], spread, ca.built, cw.built, rel_built, ca.current, cw.current, rel_current, cb.current))
    if identical:
        assert dbits(ca.built) == dbits(cw.built) and dbits(ca.current) == dbits(cw.current) and dbits(cq2.current) == dbits(cw.current)
    else:
        allowed = 2 * max(spread, 2.0 ** -52)
        assert rel_built <= allowed and rel_current <= allowed, (rel_built, rel_current, allowed)


# ---- 3. counting and the other paths ----------------------------------------------------------------------------------------
def test_counting_and_the_paths_that_end_a_build(monkeypatch):
    size, cfg = (96, 64), cfg_foveated(10, 24, (1, 2, 4))
    base = scenes.cornell_box()
    tall = base.meshes[TALL].vertex
    monkeypatch.setenv(DELAY, "150")
    # a rebuild alone on a scene that was never updated: the device copies are made, nothing moves, nothing is counted
    q = make_gpu(base, PROBE, CORNELL, size, cfg)
    want0 = render(q)
    q.update_transforms({}, rebuild="async")
    info = state(q)
    assert info.state == BUILDING and counters(info) == (1, 1, 0, 0, 0) and q.hierarchy_cost().updates == 0
    assert state(q, adopt=True).state == BUILDING and state(q).adopted == 0          # adopt on BUILDING does nothing
    info = state(q, wait=True, adopt=True)
    assert info.state == IDLE and info.adopted == 1 and q.hierarchy_cost().updates == 1
    assert np.array_equal(bits(scene_vertices(q)), bits(np.concatenate([m.vertex for m in base.meshes])))
    got = render(q)
    assert np.array_equal(bits(got[0]), bits(want0[0])) and np.array_equal(got[1], want0[1])
    q.close()                                                                        # (IDLE: nothing to join)

    r = make_gpu(base, PROBE, CORNELL, size, cfg)
    assert counters(state(r)) == (0, 0, 0, 0, 0) and state(r, adopt=True).state == IDLE          # adopt on IDLE does nothing
    new1 = {TALL: jitter(tall, 1, 6.0)}
    r.update_vertices(new1, rebuild="async")
    assert counters(state(r)) == (1, 1, 0, 0, 0)
    new2 = {SHORT: jitter(base.meshes[SHORT].vertex, 2, 5.0)}
    r.update_vertices(new2, rebuild="async")                                         # a request while BUILDING
    info = state(r)
    assert info.state == BUILDING and counters(info) == (2, 1, 0, 0, 0) and info.snapshot_update == 1
    assert state(r, wait=True).state == READY
    r.update_transforms({}, rebuild="async")                                         # a request while READY, with nothing to enqueue
    info = state(r)
    assert info.state == READY and counters(info) == (3, 1, 0, 0, 0)
    assert r.hierarchy_cost().updates == 2                                           # the two flagged calls, as their refits
    info = state(r, adopt=True)
    assert info.state == IDLE and counters(info) == (3, 1, 1, 0, 0)
    assert r.hierarchy_cost().updates == 3                                           # and the adoption
    assert state(r, adopt=True).adopted == 1
    positions = {**new1, **new2}
    fresh = make_gpu(moved(base, positions), PROBE, CORNELL, size, cfg)
    want = render(fresh)
    fresh.close()
    got = render(r)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
    # a synchronous rebuild while BUILDING discards the background result
    r.update_vertices({}, rebuild="async")
    assert counters(state(r)) == (4, 2, 1, 0, 0) and state(r).state == BUILDING and r.hierarchy_cost().updates == 3
    r.update_transforms({}, rebuild=True)
    info = state(r)
    assert info.state == IDLE and counters(info) == (4, 2, 1, 0, 1) and r.hierarchy_cost().updates == 4
    got = render(r)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
    # both rebuild bits together: refused, not counted
    with pytest.raises(lib.FovptError) as e:
        r._check(r._L.fovpt_update_vertices(r._ctx, None, 0, abi.UPDATE_REBUILD | abi.UPDATE_REBUILD_ASYNC))
    assert e.value.code == E_INVALID and counters(state(r)) == (4, 2, 1, 0, 1)
    with pytest.raises(ValueError):
        r.update_vertices({}, rebuild="later")
    # fovpt_set_scene while BUILDING
    r.update_vertices({}, rebuild="async")
    assert state(r).state == BUILDING
    md, n, td, nt, keep = scenes.pack_model(base)
    trav = C.c_uint64()
    r._check(r._L.fovpt_set_scene(r._ctx, C.cast(md, C.c_void_p), n, C.cast(td, C.c_void_p), nt, C.byref(trav)))
    r.launchParams.traversable = trav.value
    info = state(r)
    assert info.state == IDLE and counters(info) == (5, 3, 1, 0, 2)
    got = render(r)
    assert np.array_equal(bits(got[0]), bits(want0[0])) and np.array_equal(got[1], want0[1])
    r.update_vertices(new1, rebuild="async")                                         # a later update works, and so does its build
    assert state(r, wait=True).state == READY
    r.update_vertices(new2)
    info = state(r)
    assert info.state == IDLE and counters(info) == (6, 4, 2, 0, 2) and r.hierarchy_cost().updates == 3
    got = render(r)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
    n_, t_ = hierarchy(r)
    rf.check_conservative(n_, t_, rf.levels_of(n_))
    # close() while BUILDING returns
    r.update_vertices({}, rebuild="async")
    assert state(r).state == BUILDING
    r.close()


# ---- 4. rejections ------------------------------------------------------------------------------------------------------------
def test_rejections_change_nothing():
    size, cfg = (96, 64), cfg_foveated(10, 24, (1, 2, 4))
    base, r = animated_cornell(size, cfg)
    L = r._L
    ups = cornell_updates(base)
    call(r, ups[0])                                                                  # (the scene has device positions to compare)
    before = hierarchy(r)
    vtx0 = scene_vertices(r)
    acc0, px0, _ = render(r)
    st0 = r.stats()
    both = abi.UPDATE_REBUILD | abi.UPDATE_REBUILD_ASYNC
    real = {}

    def flags_of(fn_name):
        """The wrapper's own call with the flags word replaced: the entries are valid, only the flags are not."""
        fn = getattr(L, fn_name)

        def refused(*args):
            real[fn_name] = fn(*args[:-1], both)
            return real[fn_name]
        return refused

    for u, fn_name in ((ups[0], "fovpt_update_vertices"), (ups[1], "fovpt_update_transforms"), (ups[2], "fovpt_update_skinned"),
                       (ups[3], "fovpt_update_morphed"), (ups[4], "fovpt_update_animated")):
        monkey = flags_of(fn_name)
        saved = getattr(L, fn_name)
        try:
            setattr(L, fn_name, monkey)
            with pytest.raises(lib.FovptError) as e:
                call(r, u)
        finally:
            setattr(L, fn_name, saved)
        assert e.value.code == E_INVALID and real[fn_name] == E_INVALID, fn_name
        assert "FOVPT_UPDATE_REBUILD_ASYNC" in str(e.value)
    out = abi.RebuildInfo()
    assert L.fovpt_rebuild_state(r._ctx, 4, C.byref(out)) == E_INVALID              # unknown flag bits
    assert L.fovpt_rebuild_state(r._ctx, abi.REBUILD_WAIT | 8, C.byref(out)) == E_INVALID
    assert L.fovpt_rebuild_state(r._ctx, 0, None) == E_INVALID
    assert L.fovpt_rebuild_state(None, 0, C.byref(out)) == E_INVALID
    assert L.fovpt_update_vertices(r._ctx, None, 0, 4) == E_INVALID and L.fovpt_update_vertices(r._ctx, None, 0, 8) == E_INVALID
    info = state(r)
    assert info.state == IDLE and counters(info) == (0, 0, 0, 0, 0) and info.last_error == 0 and info.ms_build == 0
    after = hierarchy(r)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert np.array_equal(bits(vtx0), bits(scene_vertices(r)))
    acc1, px1, _ = render(r)
    assert np.array_equal(bits(acc0), bits(acc1)) and np.array_equal(px0, px1)
    st1 = r.stats()
    assert (st1.num_triangles, st1.num_bvh_nodes, st1.bvh_bytes, st1.tri_bytes, st1.bvh_max_depth, st1.ms_bvh_build) == \
        (st0.num_triangles, st0.num_bvh_nodes, st0.bvh_bytes, st0.tri_bytes, st0.bvh_max_depth, st0.ms_bvh_build)
    assert r.hierarchy_cost(wait=True).updates == 1                                  # the one accepted call
    r.close()
    ctx = C.c_void_p()                                                               # no scene
    lib.check(None, L.fovpt_create(C.byref(ctx), 0))
    assert L.fovpt_rebuild_state(ctx, 0, C.byref(out)) == E_NO_SCENE
    assert L.fovpt_update_vertices(ctx, None, 0, abi.UPDATE_REBUILD_ASYNC) == E_NO_SCENE
    L.fovpt_destroy(ctx)


# ---- 5. the temporal chain ----------------------------------------------------------------------------------------------------
def test_temporal_step_and_late_warp_across_an_adoption(monkeypatch):
    """A frame, a fovpt_temporal_motion step, an update, a frame and a step, then the adoption, a fovpt_warp_motion, another
    update, frame and step and another warp: colours, histories, motion vectors and warped frames are the unflagged twin's bit for
    bit -- the tracking sees no motion from the swap.  A caller's G-buffer traced before the adoption no longer goes with the
    context's hit records, which address the new hierarchy's triangle records."""
    monkeypatch.setenv(DELAY, "0")
    size = (192, 120)
    base = scenes.cornell_box()
    d = tcfg(CAPS)
    moves = [{TALL: tf.rotation_translation(12.0, (368.0, 0.0, 351.0), (-20.0, 0.0, -15.0))},
             {TALL: tf.rotation_translation(24.0, (368.0, 0.0, 351.0), (-40.0, 0.0, -30.0)), SHORT: tf.rotation_translation(-10.0, (186.0, 0.0, 168.0), (0.0, 10.0, 0.0))}]
    eye = np.asarray(CORNELL["eye"], np.float64) + np.array([6.0, 2.0, 0.0])
    to = renderer.Camera(tuple(eye), CORNELL["lookat"], CORNELL["up"], CORNELL["fovy"], size[0] / size[1])
    outs = []
    for flagged in (False, True):
        cfg = cfg_foveated(12, 36, (1, 2, 4))
        cfg.write_guides = 1
        r = make_gpu(base, PROBE, CORNELL, size, cfg)
        got = []

        def step():
            r.launchParams.frame.subframe_index = 0
            r.render()
            r.temporal_motion(d, None, None, None, r.motion_buffer())
            got.extend([bits(r.downloadTemporalColor()), bits(r.downloadTemporalHistory()), bits(r.downloadMotion()), r.downloadTemporalPixels()])

        def warp(gbuffer=None):
            r.warp_motion(to, None, gbuffer)
            got.extend([bits(r.downloadWarpedColor()), r.downloadWarpedPixels()])

        step()
        r.update_transforms(moves[0], rebuild="async" if flagged else False)
        step()
        if flagged:
            g = r.temporal_gbuffer()
            info = state(r, wait=True, adopt=True)
            assert info.adopted == 1 and info.state == IDLE
            with pytest.raises(lib.FovptError) as e:
                r.warp_motion(to, None, g)
            assert e.value.code == E_NO_FRAME
        warp()
        if flagged:
            r.update_transforms({}, rebuild="async")                                # the next adoption happens inside the update call
            assert state(r, wait=True).state == READY
        r.update_transforms(moves[1])
        if flagged:
            assert state(r).adopted == 2
        step()
        warp(r.temporal_gbuffer())                                                  # traced after the adoption: it goes with the hit records
        got.extend(gbuffer_bits(r))
        outs.append(got)
        r.close()
    assert len(outs[0]) == len(outs[1]) == 20
    for k, (a, b) in enumerate(zip(outs[1], outs[0])):
        assert np.array_equal(a, b), k
    assert (outs[1][6].view(F)[..., :2] != 0).any()                                 # the second step's motion vectors: something moved


# ---- 6. the C++ drop-in ---------------------------------------------------------------------------------------------------------
def test_cpp_dropin_rebuild_async(tmp_path):
    """SampleRenderer::updateAccel(..., REBUILD_ASYNC) / rebuildState of include/SimplePathtracer.h: request, wait, adopt and
    render; the four frames are the same pixels as Python's."""
    exe, out = build_dropin(tmp_path, "rebuild_async_gpu_test"), str(tmp_path / "rebuild_async_out.bin")
    run_dropin(exe, out)
    px = np.fromfile(out, np.uint32).reshape(4, 96, 160)
    r = dropin_renderer()
    model = r.model
    want = [render(r)[1]]
    v1 = (model.meshes[1].vertex + F([0.5, 0.0, -0.25])).astype(F)
    r.update_vertices({1: v1}, rebuild="async")
    assert state(r, wait=True).state == READY
    want.append(render(r)[1])                                                       # over the refit tree
    assert state(r, adopt=True).adopted == 1
    want.append(render(r)[1])                                                       # over the adopted one
    r.update_vertices({1: (v1 + F([-1.0, 0.25, 0.5])).astype(F)})
    want.append(render(r)[1])
    r.close()
    for k in range(4):
        assert np.array_equal(px[k], want[k]), k
    assert np.array_equal(px[1], px[2]) and not np.array_equal(px[0], px[1]) and not np.array_equal(px[2], px[3])
