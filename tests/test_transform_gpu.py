"""fovpt_update_transforms and fovpt_hierarchy_cost on the GPU.  The transforms: positions and hierarchy bytes against
tests/transform_ref.py fed to fovpt_update_vertices on the same context, frames against the CPU oracle and a fresh build of the
moved model, absolute semantics, rebuild, ordering with frames in flight, fovpt_temporal_motion's tracking, rejections.  The
cost: against refit_ref.sah_cost of the downloaded nodes within transform_ref.cost_tolerance, the counters, the two calling
modes.  And the C++ drop-in."""
import ctypes as C

import numpy as np
import pytest

import refit_ref as rf
import temporal_ref as tr
import transform_ref as tf
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer, scenes

import anim_cases as ac
from common import cfg_foveated, cfg_uniform, make_gpu
from gpu_common import bits, build_dropin, debug_buffer, run_dropin
from temporal_common import tcfg
from temporal_motion_common import vertex_arrays as motion_arrays
from test_refit_gpu import assert_frame_is_oracle, hierarchy, jitter, moved, render

pytestmark = pytest.mark.gpu
E_INVALID, E_NO_SCENE = -1, -3
CORNELL = scenes.CORNELL_CAMERA
PROBE = scenes.ambient_probe(64, 32, 2.0)
CAPS = dict(history_fovea=3, history_middle=5, history_periphery=8, history_uniform=6)      # (the default fovea keeps no history)
F = np.float32


# ---- helpers --------------------------------------------------------------------------------------------------------------
def cornell_transforms():
    """(name, {mesh: matrix}): the tall block (mesh 4) turned and carried, the short block (3) scaled unevenly, the red wall (2)
    collapsed to a point."""
    return [
        ("rigid", {4: tf.rotation_translation(23.0, (368.0, 0.0, 351.0), (-40.0, 12.0, -30.0))}),
        ("scale", {3: tf.scale_about((186.0, 0.0, 168.0), (1.3, 0.6, 0.9))}),
        ("point", {2: tf.collapse_to((552.0, 274.0, 280.0))}),
    ]


def atrium_transforms(model, seed=0):
    """A different turn about its own centre and a different carry for every mesh."""
    rng = np.random.default_rng(seed)
    return {k: tf.rotation_translation(3.0 * k + 1.0, m.vertex.astype(np.float64).mean(axis=0), rng.uniform(-6.0, 6.0, 3))
            for k, m in enumerate(model.meshes)}


def scene_vertices(r):
    p, n = debug_buffer(r, "scene_vertices")
    return r.download(p, np.empty((n // 12, 3), F))


def all_vertices(model, new=None):
    return np.concatenate([np.asarray((new or {}).get(k, m.vertex), F) for k, m in enumerate(model.meshes)])


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def dbits(x):
    return np.float64(x).view(np.uint64)


def expected_cost(r):
    """(refit_ref.sah_cost of the renderer's nodes as they are now, the tolerance for comparing the device's value with it)."""
    n, _ = hierarchy(r)
    levels = rf.levels_of(n)
    return rf.sah_cost(n, levels), tf.cost_tolerance(tf.live_entries(n, levels))


def close(got, want_tol):
    want, tol = want_tol
    return abs(got - want) <= tol * want


# ---- 1. positions ---------------------------------------------------------------------------------------------------------
def test_cornell_positions_are_the_restatement():
    model = scenes.cornell_box()
    r = renderer.SampleRenderer(model)
    ts = {}
    for _, t in cornell_transforms():
        ts.update(t)
    assert sorted(ts) == [2, 3, 4]
    r.update_transforms(ts)
    got = scene_vertices(r)
    want = all_vertices(model, tf.restate(model, ts))
    assert np.array_equal(bits(got), bits(want))
    first = np.cumsum([0] + [m.vertex.shape[0] for m in model.meshes])
    for k in (0, 1, 5):                                                   # the meshes not named keep their bits
        assert np.array_equal(bits(got[first[k]:first[k + 1]]), bits(model.meshes[k].vertex))
    assert not np.array_equal(got[first[4]:first[5]], model.meshes[4].vertex)
    r.close()


def test_atrium_positions_over_four_batches():
    model = scenes.atrium(8000)
    assert len(model.meshes) == 103                                       # three batches of 32 and a remainder of 7
    assert len({m.vertex.shape[0] for m in model.meshes}) > 3             # (with varying max_n)
    r = renderer.SampleRenderer(model)
    ts = atrium_transforms(model)
    r.update_transforms(ts)
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, tf.restate(model, ts))))
    r.close()


# ---- 2. hierarchy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cornell", "cornell_identity", "atrium"])
def test_hierarchy_is_update_vertices_of_the_restatement(case):
    """On one context (two builds of one model may order their nodes differently): fovpt_update_vertices with the restated
    positions, back to the original ones, then the transforms."""
    model = scenes.atrium(8000) if case == "atrium" else scenes.cornell_box()
    if case == "atrium":
        ts = atrium_transforms(model, 1)
    elif case == "cornell":
        ts = {k: m for _, t in cornell_transforms() for k, m in t.items()}
    else:
        ts = {k: tf.IDENTITY for k in range(len(model.meshes))}
    r = renderer.SampleRenderer(model)
    h0 = hierarchy(r)
    r.update_vertices(tf.restate(model, ts))
    want = hierarchy(r)
    r.update_vertices({k: m.vertex for k, m in enumerate(model.meshes)})
    assert same(hierarchy(r), h0)
    r.update_transforms(ts)
    assert same(hierarchy(r), want)
    if case != "cornell_identity":
        assert not same(want, h0)
    r.close()


# ---- 3. absolute ------------------------------------------------------------------------------------------------------------
def test_transforms_are_absolute_and_start_from_rest():
    model = scenes.cornell_box()
    (_, m1), (_, m2), _ = cornell_transforms()
    m2 = {4: m2[3]}                                                       # both on the tall block
    r = renderer.SampleRenderer(model)
    r.update_vertices(tf.restate(model, m2))
    want = hierarchy(r)
    r.update_vertices({4: model.meshes[4].vertex})
    r.update_transforms(m1)
    r.update_transforms(m2)                                               # M2 . rest, not M2 . M1 . rest
    assert same(hierarchy(r), want)
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, tf.restate(model, m2))))
    # a mesh fovpt_update_vertices has deformed is set from the fovpt_set_scene positions again; the other deformed mesh stays
    j3, j4 = jitter(model.meshes[3].vertex, 3, 9.0), jitter(model.meshes[4].vertex, 4, 9.0)
    r.update_vertices({3: j3, 4: j4})
    r.update_transforms(m2)
    new = tf.restate(model, m2)
    new[3] = j3
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, new)))
    r.update_vertices({3: model.meshes[3].vertex})
    assert same(hierarchy(r), want)
    r.close()


# ---- 4. frames ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["foveated", "fov_off", "guides"])
def test_cornell_frames_after_transforms(oracle, mode):
    size = (96, 64)
    cfg = cfg_uniform(2) if mode == "fov_off" else cfg_foveated(10, 24, (1, 2, 4))
    cfg.write_guides = 1 if mode == "guides" else 0
    base = scenes.cornell_box()
    r = make_gpu(base, PROBE, CORNELL, size, cfg)
    cur = base
    for name, t in cornell_transforms():
        r.update_transforms(t)
        cur = moved(cur, tf.restate(base, t))
        acc, px = assert_frame_is_oracle(oracle, r, cur, CORNELL, size, cfg)
        fresh = make_gpu(cur, PROBE, CORNELL, size, cfg)
        facc, fpx, fst = render(fresh)
        st = r.stats()
        assert np.array_equal(bits(acc), bits(facc)) and np.array_equal(px, fpx), name
        assert (st.paths, st.radiance_rays, st.shadow_rays) == (fst.paths, fst.radiance_rays, fst.shadow_rays), name
        fresh.close()
    r.close()


# ---- 5. rebuild ---------------------------------------------------------------------------------------------------------------
def test_rebuild_keeps_the_handle_and_matches_a_fresh_build():
    base = scenes.cornell_box()
    size, cfg = (96, 64), cfg_foveated(10, 24, (1, 2, 4))
    r = make_gpu(base, PROBE, CORNELL, size, cfg)
    trav, st0 = r.launchParams.traversable, r.stats()
    t = cornell_transforms()[0][1]
    r.update_transforms(t, rebuild=True)
    st1 = r.stats()
    assert r.launchParams.traversable == trav
    assert st1.ms_bvh_build != st0.ms_bvh_build and st1.num_triangles == st0.num_triangles
    n, tr_ = hierarchy(r)
    rf.check_conservative(n, tr_, rf.levels_of(n))
    fresh = make_gpu(moved(base, tf.restate(base, t)), PROBE, CORNELL, size, cfg)
    want, got = render(fresh), render(r)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
    r.update_transforms({}, rebuild=True)                                 # a rebuild alone
    got = render(r)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
    fresh.close()
    r.close()


# ---- 6. no synchronisation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["frames_in_flight", "chains_per_frame"])
def test_transforms_between_frames_in_flight(mode):
    import torch
    size = (192, 128)
    cfg = cfg_foveated(20, 48, (2, 4, 8))                   # >= 16384 sample slots: chains_per_frame = 2 does split the frame
    if mode == "frames_in_flight":
        cfg.frames_in_flight = 2
    else:
        cfg.chains_per_frame = 2
    base = scenes.cornell_box()
    poses = [{4: tf.rotation_translation(6.0 * k, (368.0, 0.0, 351.0), (-8.0 * k, 0.0, -5.0 * k))} for k in range(8)]
    shape = (size[1], size[0])

    def buffers():
        return (torch.zeros(shape + (4,), dtype=torch.float32, device="cuda"), torch.zeros(shape, dtype=torch.int32, device="cuda"))

    def issue(r, bufs):
        f = r.launchParams.frame
        f.accum_buffer, f.frame_buffer = bufs[0].data_ptr(), bufs[1].data_ptr()
        f.subframe_index = 0
        r.render_async()

    r = make_gpu(base, PROBE, CORNELL, size, cfg)           # each pose alone, a synchronisation after it
    want = []
    for p in poses:
        b = buffers()
        torch.cuda.synchronize()
        r.update_transforms(p)
        issue(r, b)
        r.synchronize()
        want.append((b[0].cpu().numpy(), b[1].cpu().numpy()))
    r.close()
    r = make_gpu(base, PROBE, CORNELL, size, cfg)           # back to back
    outs = [buffers() for _ in poses]
    torch.cuda.synchronize()
    for p, b in zip(poses, outs):
        r.update_transforms(p)
        issue(r, b)
    r.synchronize()
    for k, (b, w) in enumerate(zip(outs, want)):
        assert np.array_equal(bits(b[0].cpu().numpy()), bits(w[0])) and np.array_equal(b[1].cpu().numpy(), w[1]), "pose %d" % k
    assert not np.array_equal(want[0][1], want[7][1])
    r.close()


# ---- 7. temporal ----------------------------------------------------------------------------------------------------------
def test_temporal_motion_sees_transforms_as_vertex_updates():
    size = (192, 120)
    base = scenes.cornell_box()
    t = cornell_transforms()[0][1]
    d = tcfg(CAPS)
    outs = []
    for use_transforms in (True, False):
        cfg = cfg_foveated(12, 36, (1, 2, 4))
        cfg.write_guides = 1
        r = make_gpu(base, PROBE, CORNELL, size, cfg)
        r.render()
        r.temporal_motion(d, None, None, None, r.motion_buffer())
        if use_transforms:
            r.update_transforms(t)
        else:
            r.update_vertices(tf.restate(base, t))
        r.launchParams.frame.subframe_index = 0
        r.render()
        r.temporal_motion(d, None, None, None, r.motion_buffer())
        outs.append((r.downloadTemporalColor(), r.downloadTemporalHistory(), r.downloadMotion(), r.downloadTemporalPixels(),
                     r.downloadGBuffer()["prim"]))
        r.close()
    a, b = outs
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(bits(x), bits(y))
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    mesh_of_prim = motion_arrays(base)[2]
    prim = a[4]
    on_block = (prim != tr.MISS) & (mesh_of_prim[np.where(prim == tr.MISS, 0, prim).astype(np.int64)] == 4)
    assert on_block.sum() > 100 and (a[1][on_block][:, 3] > 1).mean() > 0.5


# ---- 8. rejections ------------------------------------------------------------------------------------------------------------
def test_rejections_change_nothing():
    size, cfg = (64, 48), cfg_foveated(8, 20, (1, 2, 4))
    base = scenes.cornell_box()
    r = make_gpu(base, PROBE, CORNELL, size, cfg)
    L = r._L
    before = hierarchy(r)
    acc0, px0, _ = render(r)
    st0 = r.stats()
    good = ac.TRANSFORM_GOOD

    def call(entries, n=None, flags=0):
        return L.fovpt_update_transforms(r._ctx, ac.pack_transforms(entries), len(entries) if n is None else n, flags)

    def with_entry(i, v):
        return ac.with_entry(good, i, v).reshape(-1)

    for what, entries, n, flags, _ in ac.transform_cases(base):
        assert call(entries, n, flags) == E_INVALID, (what, n, flags)
        ac.assert_recorded("transforms", what, E_INVALID, L.fovpt_last_error(r._ctx))
    assert 400 < np.abs(base.meshes[4].vertex).max() < 500
    assert call([(4, with_entry(2, 1e35))]) == 0                  # a tenth of it is below the bound: finite, if absurd ...
    assert np.isfinite(scene_vertices(r)).all()
    r.update_vertices({4: base.meshes[4].vertex})                 # ... and back
    assert L.fovpt_update_transforms(r._ctx, None, 1, 0) == E_INVALID
    assert L.fovpt_update_transforms(None, None, 0, 0) == E_INVALID
    assert L.fovpt_update_transforms(r._ctx, None, 0, 0) == 0     # nothing to do
    assert L.fovpt_update_vertices(r._ctx, None, 0, 4) == E_INVALID   # (fovpt_update_vertices still refuses unknown bits)
    out = abi.HierarchyCost()
    assert L.fovpt_hierarchy_cost(r._ctx, 2, C.byref(out)) == E_INVALID
    assert L.fovpt_hierarchy_cost(r._ctx, 0, None) == E_INVALID
    assert L.fovpt_hierarchy_cost(None, 0, C.byref(out)) == E_INVALID
    after = hierarchy(r)
    assert same(before, after)
    acc1, px1, _ = render(r)
    assert np.array_equal(bits(acc0), bits(acc1)) and np.array_equal(px0, px1)
    st1 = r.stats()
    assert (st1.num_triangles, st1.num_bvh_nodes, st1.bvh_bytes, st1.tri_bytes, st1.bvh_max_depth, st1.ms_bvh_build) == \
        (st0.num_triangles, st0.num_bvh_nodes, st0.bvh_bytes, st0.tri_bytes, st0.bvh_max_depth, st0.ms_bvh_build)
    assert r.hierarchy_cost(wait=True).updates == 2               # the two accepted calls, none of the refused ones
    for bad in (np.diag(F([1, 1, 1, 2])), np.eye(4, dtype=F)[::-1], np.eye(3, dtype=F)):     # the wrapper's own checks
        with pytest.raises(ValueError):
            r.update_transforms({0: bad})
    r.update_transforms({0: np.eye(4, dtype=F)})
    r.close()
    ctx = C.c_void_p()                                            # no scene
    lib.check(None, L.fovpt_create(C.byref(ctx), 0))
    assert L.fovpt_update_transforms(ctx, None, 0, 0) == E_NO_SCENE
    assert L.fovpt_hierarchy_cost(ctx, 0, C.byref(out)) == E_NO_SCENE
    L.fovpt_destroy(ctx)


# ---- 9. cost --------------------------------------------------------------------------------------------------------------
def test_hierarchy_cost_follows_the_tree():
    model = scenes.atrium(8000)
    r = renderer.SampleRenderer(model)
    c0 = r.hierarchy_cost()
    assert dbits(c0.built) == dbits(c0.current) and (c0.updates, c0.measured) == (0, 0)
    want0 = expected_cost(r)
    assert close(c0.built, want0), (c0.built, want0)
    assert want0[0] > 1.0 and want0[1] < 1e-11
    # the largest mesh carried 0.8 of the scene's extent away: the refit tree's cost rises
    lo = np.min([m.vertex.min(axis=0) for m in model.meshes], axis=0)
    hi = np.max([m.vertex.max(axis=0) for m in model.meshes], axis=0)
    k = int(np.argmax([m.index.shape[0] for m in model.meshes]))
    carry = np.concatenate([np.eye(3), ((hi - lo) * 0.8).astype(np.float64)[:, None]], axis=1).astype(F)
    r.update_transforms({k: carry})
    c1 = r.hierarchy_cost(wait=True)
    assert (c1.updates, c1.measured) == (1, 1) and dbits(c1.built) == dbits(c0.built)
    want1 = expected_cost(r)
    assert close(c1.current, want1), (c1.current, want1)
    assert c1.current > c1.built
    # a second update through the other entry point, polled at once: whichever measurement the poll returns, the pair matches
    r.update_vertices({1: jitter(model.meshes[1].vertex, 5, 30.0)})
    c2 = r.hierarchy_cost()
    assert c2.updates == 2 and c2.measured in (1, 2)
    want2 = expected_cost(r)
    if c2.measured == 1:
        assert dbits(c2.current) == dbits(c1.current)
    else:
        assert close(c2.current, want2), (c2.current, want2)
    c3 = r.hierarchy_cost(wait=True)
    assert (c3.updates, c3.measured) == (2, 2) and close(c3.current, want2), (c3.current, want2)
    assert dbits(c3.current) != dbits(c1.current)
    c4 = r.hierarchy_cost(wait=True)                               # two waits in a row: identical bits
    assert bytes(c3) == bytes(c4)
    # a rebuild: a new `built`, and current is it
    r.update_transforms({}, rebuild=True)
    c5 = r.hierarchy_cost()
    assert (c5.updates, c5.measured) == (3, 3) and dbits(c5.built) == dbits(c5.current)
    assert close(c5.built, expected_cost(r)) and dbits(c5.built) != dbits(c0.built)
    r.close()


def test_hierarchy_cost_before_watching_and_with_every_slot_in_flight():
    model = scenes.atrium(8000)
    r = renderer.SampleRenderer(model)
    ts = atrium_transforms(model, 2)
    r.update_transforms(ts)                                        # nobody is watching: no measurement follows
    c = r.hierarchy_cost()                                         # the first call: never blocks, may still hold the build's pair
    assert c.updates == 1 and c.measured in (0, 1)
    if c.measured == 0:
        assert dbits(c.current) == dbits(c.built)
    c = r.hierarchy_cost(wait=True)
    assert (c.updates, c.measured) == (1, 1) and close(c.current, expected_cost(r))
    for k in range(12):                                            # more updates back to back than there are result slots
        r.update_transforms({k: ts[k + 1]})
    c = r.hierarchy_cost()
    assert c.updates == 13 and 1 <= c.measured <= 13
    c = r.hierarchy_cost(wait=True)
    assert (c.updates, c.measured) == (13, 13) and close(c.current, expected_cost(r))
    # fovpt_set_scene starts over
    md, n, td, nt, keep = scenes.pack_model(model)
    trav = C.c_uint64()
    r._check(r._L.fovpt_set_scene(r._ctx, C.cast(md, C.c_void_p), n, C.cast(td, C.c_void_p), nt, C.byref(trav)))
    c = r.hierarchy_cost()
    assert (c.updates, c.measured) == (0, 0) and dbits(c.built) == dbits(c.current) and close(c.built, expected_cost(r))
    r.update_transforms({0: ts[0]})                                # the rest positions are made again for the new scene
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, tf.restate(model, {0: ts[0]}))))
    r.close()


# ---- 10. C++ ------------------------------------------------------------------------------------------------------------------
def test_cpp_update_transforms(tmp_path):
    """SampleRenderer::updateTransforms / hierarchyCost of include/SimplePathtracer.h: the pixels of a fresh renderer over the
    moved Model after a refit and after a rebuild."""
    exe, out = build_dropin(tmp_path, "transform_gpu_test"), str(tmp_path / "transform_out.bin")
    run_dropin(exe, out)
    px = np.fromfile(out, np.uint32).reshape(4, 96, 160)
    assert np.array_equal(px[0], px[1]) and np.array_equal(px[2], px[3])     # refit / rebuild == fresh renderer
    assert not np.array_equal(px[0], px[2])
