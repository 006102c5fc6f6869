"""fovpt_set_skins and fovpt_update_skinned on the GPU: positions and hierarchy bytes against tests/skin_ref.py fed to
fovpt_update_vertices on the same context, frames against the CPU oracle and a fresh build of the moved model, absolute
semantics, device matrices, ordering with frames in flight, rebuild and the cost counters, fovpt_temporal_motion's tracking, the
life cycle of a skin, rejections, a seeded sweep, and the C++ drop-in.  FOVPT_FUZZSK_TO widens the sweep."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import skin_ref as sk
import temporal_ref as tr
import transform_ref as tf
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer, scenes

import anim_cases as ac
from anim_cases import cornell_poses, cornell_skins
from common import cfg_foveated, cfg_uniform, make_gpu
from gpu_common import bits, build_dropin, debug_buffer, dropin_renderer, run_dropin
from temporal_common import tcfg
from temporal_motion_common import vertex_arrays as motion_arrays
from test_refit_gpu import assert_frame_is_oracle, hierarchy, jitter, moved, oracle_frame, render

pytestmark = pytest.mark.gpu
E_INVALID, E_NO_SCENE = -1, -3
CORNELL = scenes.CORNELL_CAMERA
PROBE = scenes.ambient_probe(64, 32, 2.0)
CAPS = dict(history_fovea=3, history_middle=5, history_periphery=8, history_uniform=6)      # (the default fovea keeps no history)
F = np.float32
SEEDS = range(0, int(os.environ.get("FOVPT_FUZZSK_TO", "8")))


# ---- helpers --------------------------------------------------------------------------------------------------------------
def atrium_skins(model, big=None):
    """Every mesh skinned, joint counts cycling 1, 2, 5 and 17; mesh `big` over FOVPT_SKIN_MAX_JOINTS joints."""
    return {k: sk.bend(m.vertex, sk.MAX_JOINTS if k == big else (1, 2, 5, 17)[k % 4]) for k, m in enumerate(model.meshes)}


def atrium_poses(model, skins, seed=0):
    rng = np.random.default_rng(seed)
    return {k: sk.bend_pose(model.meshes[k].vertex, s[2], 3.0 * k + 1.0, rng.uniform(-6.0, 6.0, 3)) for k, s in skins.items()}


def scene_vertices(r):
    p, n = debug_buffer(r, "scene_vertices")
    return r.download(p, np.empty((n // 12, 3), F))


def all_vertices(model, new=None):
    return np.concatenate([np.asarray((new or {}).get(k, m.vertex), F) for k, m in enumerate(model.meshes)])


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def rest_of(model):
    return {k: m.vertex for k, m in enumerate(model.meshes)}


# ---- 1. positions ---------------------------------------------------------------------------------------------------------
def test_cornell_positions_are_the_restatement():
    model = scenes.cornell_box()
    r = renderer.SampleRenderer(model)
    skins, poses = cornell_skins(model), cornell_poses(model)
    r.set_skins(skins)
    r.update_skinned(poses)
    got = scene_vertices(r)
    want = all_vertices(model, sk.restate(model, skins, poses))
    assert np.array_equal(bits(got), bits(want))
    first = np.cumsum([0] + [m.vertex.shape[0] for m in model.meshes])
    for k in (0, 1, 2, 5):                                                # the meshes not named keep their bits
        assert np.array_equal(bits(got[first[k]:first[k + 1]]), bits(model.meshes[k].vertex))
    for k in (3, 4):
        assert not np.array_equal(got[first[k]:first[k + 1]], model.meshes[k].vertex)
    r.update_skinned({4: poses[4]})                                       # one of the two: the other keeps what it last had
    assert np.array_equal(bits(scene_vertices(r)), bits(want))
    r.close()


# ---- 2. batches -----------------------------------------------------------------------------------------------------------
def test_atrium_positions_over_four_batches():
    model = scenes.atrium(8000)
    assert len(model.meshes) == 103                                       # three batches of 32 and a remainder of 7
    nv = [m.vertex.shape[0] for m in model.meshes]
    assert len(set(nv)) > 3 and min(nv) <= 8 and any(n % 256 for n in nv)  # varying max_n, tiny meshes, no multiple of the block
    big = int(np.argmax(nv))
    skins = atrium_skins(model, big)
    assert skins[big][0].max() == sk.MAX_JOINTS - 1                       # the last joint of the largest palette is used
    assert sorted({s[2] for s in skins.values()}) == [1, 2, 5, 17, sk.MAX_JOINTS]
    poses = atrium_poses(model, skins)
    r = renderer.SampleRenderer(model)
    r.set_skins(skins)
    r.update_skinned(poses)
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, sk.restate(model, skins, poses))))
    r.close()


def test_a_mesh_of_several_blocks():
    """The atrium's meshes have at most 169 vertices: one block each.  A sheet of 27 x 26 = 702 vertices takes three blocks, the
    last one partly filled, beside a mesh of 4."""
    nu, nv = 27, 26
    u, v = np.meshgrid(np.arange(nu, dtype=F), np.arange(nv, dtype=F), indexing="ij")
    sheet = np.stack([u * F(0.5), v * F(0.75), np.sin(u * F(0.4)) + F(0.25) * v], axis=-1).reshape(-1, 3).astype(F)
    q = (np.arange(nu - 1)[:, None] * nv + np.arange(nv - 1)[None, :]).reshape(-1)
    idx = np.concatenate([np.stack([q, q + nv, q + nv + 1], axis=1), np.stack([q, q + nv + 1, q + 1], axis=1)]).astype(np.uint32)
    floor = scenes.cornell_box().meshes[1]
    mat = floor.material
    model = scenes.Model([floor, scenes.TriangleMesh(sheet, idx, mat, np.zeros((len(sheet), 2), F), -1)])
    assert len(sheet) == 702 and len(sheet) > 2 * 256 and len(sheet) % 256
    skins = {1: sk.bend(sheet, 7), 0: sk.bend(floor.vertex, 2)}
    poses = {1: sk.bend_pose(sheet, 7, 80.0, (3.0, 1.0, -2.0)), 0: sk.bend_pose(floor.vertex, 2, 10.0, (0.0, 5.0, 0.0))}
    r = renderer.SampleRenderer(model)
    r.set_skins(skins)
    r.update_skinned(poses)
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, sk.restate(model, skins, poses))))
    r.close()


# ---- 3. hierarchy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cornell", "cornell_identity", "atrium"])
def test_hierarchy_is_update_vertices_of_the_restatement(case):
    """On one context (two builds of one model may order their nodes differently): fovpt_update_vertices with the restated
    positions, back to the original ones, then the poses."""
    model = scenes.atrium(8000) if case == "atrium" else scenes.cornell_box()
    if case == "atrium":
        skins = atrium_skins(model)
        poses = atrium_poses(model, skins, 1)
    elif case == "cornell":
        skins, poses = cornell_skins(model), cornell_poses(model)
    else:
        skins = {k: sk.bend(m.vertex, 2) for k, m in enumerate(model.meshes)}
        poses = {k: np.tile(tf.IDENTITY, (2, 1, 1)) for k in skins}
    r = renderer.SampleRenderer(model)
    r.set_skins(skins)
    h0 = hierarchy(r)
    r.update_vertices(sk.restate(model, skins, poses))
    want = hierarchy(r)
    r.update_vertices(rest_of(model))
    assert same(hierarchy(r), h0)
    r.update_skinned(poses)
    assert same(hierarchy(r), want)
    if case != "cornell_identity":
        assert not same(want, h0)
    r.close()


# ---- 4. one joint ---------------------------------------------------------------------------------------------------------
def test_one_joint_of_weight_one_is_update_transforms():
    """(A matrix without zero entries: test_skin_cpu.py says why.)"""
    model = scenes.cornell_box()
    m = sk.dense_matrix()
    r = renderer.SampleRenderer(model)
    r.set_skins({4: sk.bend(model.meshes[4].vertex, 1)})
    r.update_transforms({4: m})
    want_v, want_h = scene_vertices(r), hierarchy(r)
    r.update_vertices({4: model.meshes[4].vertex})
    assert not same(hierarchy(r), want_h)
    r.update_skinned({4: m[None]})
    assert np.array_equal(bits(scene_vertices(r)), bits(want_v)) and same(hierarchy(r), want_h)
    r.close()


# ---- 5. frames ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["foveated", "fov_off"])
def test_cornell_frames_after_a_pose(oracle, mode):
    size = (96, 64)
    cfg = cfg_uniform(2) if mode == "fov_off" else cfg_foveated(10, 24, (1, 2, 4))
    base = scenes.cornell_box()
    skins, poses = cornell_skins(base), cornell_poses(base)
    r = make_gpu(base, PROBE, CORNELL, size, cfg)
    acc0, px0, _ = render(r)
    r.set_skins(skins)
    acc1, px1, _ = render(r)                                              # a skin alone moves nothing
    assert np.array_equal(bits(acc0), bits(acc1)) and np.array_equal(px0, px1)
    r.update_skinned(poses)
    cur = moved(base, sk.restate(base, skins, poses))
    acc, px = assert_frame_is_oracle(oracle, r, cur, CORNELL, size, cfg)
    fresh = make_gpu(cur, PROBE, CORNELL, size, cfg)
    facc, fpx, fst = render(fresh)
    st = r.stats()
    assert np.array_equal(bits(acc), bits(facc)) and np.array_equal(px, fpx)
    assert (st.paths, st.radiance_rays, st.shadow_rays) == (fst.paths, fst.radiance_rays, fst.shadow_rays)
    assert not np.array_equal(px, px0)
    fresh.close()
    r.close()


# ---- 6. absolute ------------------------------------------------------------------------------------------------------------
def test_poses_are_absolute_and_start_from_rest():
    model = scenes.cornell_box()
    skins, p1, p2 = cornell_skins(model), cornell_poses(model, 1.0), cornell_poses(model, 0.4)
    r = renderer.SampleRenderer(model)
    r.set_skins(skins)
    r.update_vertices(sk.restate(model, skins, p2))
    want = hierarchy(r)
    want_v = all_vertices(model, sk.restate(model, skins, p2))
    r.update_vertices(rest_of(model))
    r.update_skinned(p1)
    r.update_skinned(p2)                                                  # P2 of rest, not P2 of P1 of rest
    assert same(hierarchy(r), want) and np.array_equal(bits(scene_vertices(r)), bits(want_v))
    # a mesh fovpt_update_vertices has deformed is set from the fovpt_set_scene positions again; another deformed mesh stays
    j2, j4 = jitter(model.meshes[2].vertex, 3, 9.0), jitter(model.meshes[4].vertex, 4, 9.0)
    r.update_vertices({2: j2, 4: j4})
    r.update_skinned(p2)
    new = sk.restate(model, skins, p2)
    new[2] = j2
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, new)))
    r.update_vertices({2: model.meshes[2].vertex})
    assert same(hierarchy(r), want)
    # a pose, then fovpt_update_transforms on the same (still skinned) mesh: the transform of rest alone
    m = sk.dense_matrix()
    r.update_transforms({4: m})
    new = sk.restate(model, skins, p2)
    new[4] = tf.apply(model.meshes[4].vertex, m)
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, new)))
    r.update_skinned({4: p1[4]})                                          # ... and back under the skin
    new[4] = sk.apply(model.meshes[4].vertex, skins[4][0], skins[4][1], p1[4])
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, new)))
    r.close()


# ---- 7. device matrices -----------------------------------------------------------------------------------------------------
def test_device_matrices_give_the_host_bytes():
    import torch
    model = scenes.atrium(8000)
    skins = atrium_skins(model)
    poses = atrium_poses(model, skins, 2)
    r = renderer.SampleRenderer(model)
    r.set_skins(skins)
    r.update_skinned(poses)
    want_v, want_h = scene_vertices(r), hierarchy(r)
    r.update_vertices(rest_of(model))
    assert not same(hierarchy(r), want_h)
    dev = {k: torch.from_numpy(np.ascontiguousarray(p, F)).cuda() for k, p in poses.items()}
    torch.cuda.synchronize()
    r.update_skinned(dev)
    assert np.array_equal(bits(scene_vertices(r)), bits(want_v)) and same(hierarchy(r), want_h)
    with pytest.raises(ValueError):
        r.update_skinned({0: poses[0], 1: dev[1]})
    with pytest.raises(ValueError):
        r.update_skinned({0: dev[0].reshape(-1, 12)})
    r.close()


# ---- 8. frames in flight ------------------------------------------------------------------------------------------------------
def test_poses_between_frames_in_flight(oracle):
    import torch
    size = (96, 64)
    cfg = cfg_foveated(10, 24, (1, 2, 4))
    cfg.frames_in_flight = 2
    base = scenes.cornell_box()
    skins = cornell_skins(base)
    poses = [cornell_poses(base, k) for k in (0.3, 0.65, 1.0)]
    shape = (size[1], size[0])
    r = make_gpu(base, PROBE, CORNELL, size, cfg)
    r.set_skins(skins)
    outs = [(torch.zeros(shape + (4,), dtype=torch.float32, device="cuda"), torch.zeros(shape, dtype=torch.int32, device="cuda")) for _ in poses]
    torch.cuda.synchronize()
    for p, b in zip(poses, outs):                                         # pose, frame, pose, frame, pose, frame: no synchronisation
        r.update_skinned(p)
        f = r.launchParams.frame
        f.accum_buffer, f.frame_buffer = b[0].data_ptr(), b[1].data_ptr()
        f.subframe_index = 0
        r.render_async()
    r.synchronize()
    frames = []
    for k, (p, b) in enumerate(zip(poses, outs)):
        Fr, _ = oracle_frame(oracle, moved(base, sk.restate(base, skins, p)), CORNELL, size, cfg)
        acc, px = b[0].cpu().numpy(), b[1].cpu().numpy()
        assert np.array_equal(bits(acc), bits(Fr.accum)) and np.array_equal(px.view(np.uint32), Fr.frame), "pose %d" % k
        frames.append(px)
    assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[1], frames[2])
    r.close()


# ---- 9. rebuild -----------------------------------------------------------------------------------------------------------
def test_rebuild_and_the_cost_counters():
    base = scenes.cornell_box()
    size, cfg = (96, 64), cfg_foveated(10, 24, (1, 2, 4))
    skins, poses = cornell_skins(base), cornell_poses(base)
    r = make_gpu(base, PROBE, CORNELL, size, cfg)
    trav = r.launchParams.traversable
    r.set_skins(skins)
    assert r.hierarchy_cost().updates == 0                                # a skin is no update
    r.update_skinned(poses)
    c1 = r.hierarchy_cost(wait=True)
    assert (c1.updates, c1.measured) == (1, 1)                            # a refit pose is counted ...
    refit = render(r)
    r.update_skinned(poses, rebuild=True)
    c2 = r.hierarchy_cost()
    assert (c2.updates, c2.measured) == (2, 2) and c2.current == c2.built  # ... and so is a rebuild, which measures at once
    assert r.launchParams.traversable == trav
    rebuilt = render(r)
    assert np.array_equal(bits(refit[0]), bits(rebuilt[0])) and np.array_equal(refit[1], rebuilt[1])
    fresh = make_gpu(moved(base, sk.restate(base, skins, poses)), PROBE, CORNELL, size, cfg)
    want = render(fresh)
    assert np.array_equal(bits(rebuilt[0]), bits(want[0])) and np.array_equal(rebuilt[1], want[1])
    r.update_skinned({}, rebuild=True)                                    # a rebuild alone
    assert r.hierarchy_cost().updates == 3
    r.update_skinned({})                                                  # nothing to do: not counted
    assert r.hierarchy_cost().updates == 3
    r.update_skinned(cornell_poses(base, 0.5))
    c3 = r.hierarchy_cost(wait=True)
    assert (c3.updates, c3.measured) == (4, 4)
    fresh.close()
    r.close()


# ---- 10. temporal ---------------------------------------------------------------------------------------------------------
def test_temporal_motion_sees_poses_as_vertex_updates():
    size = (192, 120)
    base = scenes.cornell_box()
    skins, poses = cornell_skins(base), cornell_poses(base, 0.5)
    d = tcfg(CAPS)
    outs = []
    for use_skin in (True, False):
        cfg = cfg_foveated(12, 36, (1, 2, 4))
        cfg.write_guides = 1
        r = make_gpu(base, PROBE, CORNELL, size, cfg)
        r.set_skins(skins)
        r.render()
        r.temporal_motion(d, None, None, None, r.motion_buffer())
        if use_skin:
            r.update_skinned(poses)
        else:
            r.update_vertices(sk.restate(base, skins, poses))
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


# ---- 11. the life cycle of a skin -------------------------------------------------------------------------------------------
def test_set_skins_replaces_removes_and_ends_with_the_scene():
    model = scenes.cornell_box()
    v4 = model.meshes[4].vertex
    r = renderer.SampleRenderer(model)
    skins = cornell_skins(model)
    r.set_skins(skins)
    poses = cornell_poses(model)
    r.update_skinned(poses)
    # replace mesh 4's skin (another joint count: the layout of mesh 3's moves too); mesh 3's stays
    rng = np.random.default_rng(3)
    new4 = sk.random_skin(rng, len(v4), 6)
    r.set_skins({4: new4})
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, sk.restate(model, skins, poses))))     # geometry does not move
    skins[4] = new4
    poses[4] = sk.random_pose(rng, v4, 6)
    r.update_skinned(poses)
    want = all_vertices(model, sk.restate(model, skins, poses))
    assert np.array_equal(bits(scene_vertices(r)), bits(want))
    ps = (abi.SkinPose * 1)()
    old = np.ascontiguousarray(cornell_poses(model)[4])
    ps[0].mesh, ps[0].num_joints, ps[0].matrices = 4, 3, old.ctypes.data
    assert r._L.fovpt_update_skinned(r._ctx, ps, 1, 0) == E_INVALID       # the old joint count
    # remove mesh 3's skin: a pose for it is refused, mesh 4 still poses
    h = hierarchy(r)
    r.set_skins({3: None})
    with pytest.raises(lib.FovptError):
        r.update_skinned({3: poses[3]})
    with pytest.raises(lib.FovptError):
        r.update_skinned(poses)                                           # ... also beside a good one: all or nothing
    assert np.array_equal(bits(scene_vertices(r)), bits(want)) and same(hierarchy(r), h)
    p4 = {4: sk.random_pose(rng, v4, 6)}
    r.update_skinned(p4)
    new = sk.restate(model, skins, poses)
    new[4] = sk.restate(model, skins, p4)[4]
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, new)))
    r.set_skins({4: None})                                                # the last skin goes
    with pytest.raises(lib.FovptError):
        r.update_skinned(p4)
    r.set_skins({4: new4})
    # fovpt_set_scene drops every skin
    md, n, td, nt, keep = scenes.pack_model(model)
    trav = C.c_uint64()
    r._check(r._L.fovpt_set_scene(r._ctx, C.cast(md, C.c_void_p), n, C.cast(td, C.c_void_p), nt, C.byref(trav)))
    for k in (3, 4):
        with pytest.raises(lib.FovptError):
            r.update_skinned({k: poses[k]})
    r.set_skins({4: new4})                                                # and a new scene takes new ones
    r.update_skinned(p4)
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, sk.restate(model, skins, p4))))
    r.close()


# ---- 12. rejections -------------------------------------------------------------------------------------------------------
def test_rejections_change_nothing():
    base = scenes.cornell_box()
    r = renderer.SampleRenderer(base)
    L = r._L
    n4 = base.meshes[4].vertex.shape[0]
    skins = ac.skin_scene(base)                                           # S = 4 on mesh 3, S = 1 on mesh 5
    r.set_skins(skins)
    poses = cornell_poses(base)
    r.update_skinned(poses)
    before_v, before_h = scene_vertices(r), hierarchy(r)

    def unchanged():
        return np.array_equal(bits(scene_vertices(r)), bits(before_v)) and same(hierarchy(r), before_h)

    # -- fovpt_set_skins
    j4, wt4 = np.ascontiguousarray(skins[4][0]), np.ascontiguousarray(skins[4][1])

    for what, entries, n in ac.skin_set_cases(base, skins):
        assert L.fovpt_set_skins(r._ctx, ac.pack_skins(entries), len(entries) if n is None else n) == E_INVALID, what
        ac.assert_recorded("skins", what, E_INVALID, L.fovpt_last_error(r._ctx))
        assert unchanged(), what
    assert L.fovpt_set_skins(r._ctx, None, 1) == E_INVALID
    assert L.fovpt_set_skins(None, None, 0) == E_INVALID
    assert L.fovpt_set_skins(r._ctx, None, 0) == 0                        # nothing to do
    for bad in ((np.zeros((n4, 3), np.uint16), wt4), (j4, wt4[:-1]), (j4.astype(np.float32), wt4), (j4.astype(np.int64) + 70000, wt4)):
        with pytest.raises(ValueError):                                   # the wrapper's own checks
            r.set_skins({4: bad})
    r.update_skinned(poses)                                               # the skins are the ones set before the refused calls
    assert unchanged()

    # -- fovpt_update_skinned
    P4, P3, P5 = np.ascontiguousarray(poses[4]), np.ascontiguousarray(poses[3]), np.tile(tf.IDENTITY, (1, 1, 1))

    def pose(mesh=4, nj=3, m=P4):
        return dict(mesh=mesh, nj=nj, m=m)

    def update(entries, n=None, flags=0, ctx=r._ctx):
        return L.fovpt_update_skinned(ctx, ac.pack_skin_poses(entries), len(entries) if n is None else n, flags)

    row_only = ac.row_only
    for what, entries, n, flags, _ in ac.skin_pose_cases(base, poses):
        assert update(entries, n, flags) == E_INVALID, (what, n, flags)
        ac.assert_recorded("skinned", what, E_INVALID, L.fovpt_last_error(r._ctx))
        assert unchanged(), what
    assert L.fovpt_update_skinned(r._ctx, None, 1, 0) == E_INVALID
    assert L.fovpt_update_skinned(None, None, 0, 0) == E_INVALID
    assert L.fovpt_update_skinned(r._ctx, None, 0, 0) == 0                # nothing to do
    assert unchanged()
    assert r.hierarchy_cost(wait=True).updates == 2                       # the two accepted calls, none of the refused ones
    for bad in (np.zeros((3, 4), F), np.zeros((3, 3, 3), F), np.tile(np.diag(F([1, 1, 1, 2])), (3, 1, 1))):       # the wrapper's own checks
        with pytest.raises(ValueError):
            r.update_skinned({4: bad})
    r.update_skinned({4: np.tile(np.eye(4, dtype=F), (3, 1, 1))})         # the (J, 4, 4) form
    r.update_skinned({4: P4})
    assert unchanged()
    # -- exactly 2^127 is not above: accepted, finite, and the restatement's
    cur = sk.restate(base, skins, {3: P3, 4: P4})                         # (mesh 5 is still where fovpt_set_scene put it)
    for mesh, t in ((5, F(2.0 ** 127)), (3, F(2.0 ** 125))):
        m = row_only(t)
        assert sk.overflow_bound(base.meshes[mesh].vertex, skins[mesh][1], m) == 2.0 ** 127
        assert sk.accepted(base.meshes[mesh].vertex, skins[mesh][1], m)
        assert update([pose(mesh=mesh, nj=1, m=m)]) == 0
        cur[mesh] = sk.restate(base, skins, {mesh: m})[mesh]
        got = scene_vertices(r)
        assert np.isfinite(got).all() and (got == F(2.0 ** 127)).any()
        assert np.array_equal(bits(got), bits(all_vertices(base, cur)))
    r.close()
    ctx = C.c_void_p()                                                    # no scene
    lib.check(None, L.fovpt_create(C.byref(ctx), 0))
    assert L.fovpt_set_skins(ctx, None, 0) == E_NO_SCENE
    assert L.fovpt_update_skinned(ctx, None, 0, 0) == E_NO_SCENE
    L.fovpt_destroy(ctx)


# ---- 13. a seeded sweep -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep_scene():
    model = scenes.atrium(2000)
    r = renderer.SampleRenderer(model)
    yield model, r, hierarchy(r)
    r.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_skins_and_poses(sweep_scene, seed):
    model, r, h0 = sweep_scene
    nmesh = len(model.meshes)
    assert nmesh > 32 and nmesh % 32 != 0
    rng = np.random.default_rng(1000 + seed)
    named = [k for k in range(nmesh) if rng.uniform() < (1.0 if seed % 4 == 0 else 0.6)]      # every fourth seed: all of them
    skins = {k: sk.random_skin(rng, model.meshes[k].vertex.shape[0], int(rng.integers(1, 10))) for k in named}
    r.set_skins({k: skins.get(k) for k in range(nmesh)})                  # (the others lose what an earlier seed gave them)
    posed = [k for k in named if rng.uniform() < 0.8] or named[:1]
    poses = {k: sk.random_pose(rng, model.meshes[k].vertex, skins[k][2]) for k in posed}
    w = np.concatenate([skins[k][1] for k in posed])
    assert (w == 0).any() and (np.abs(w.astype(np.float64).sum(axis=1) - 1) > 0.05).any()
    for k in posed:                                                       # every drawn case is within the rule: none is skipped
        assert sk.accepted(model.meshes[k].vertex, skins[k][1], poses[k]), k
    want_v = sk.restate(model, skins, poses)
    r.update_vertices(rest_of(model))
    assert same(hierarchy(r), h0)
    r.update_vertices(want_v)
    want_h = hierarchy(r)
    r.update_vertices(rest_of(model))
    r.update_skinned(poses)
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, want_v)))
    assert same(hierarchy(r), want_h) and not same(want_h, h0)


# ---- 14. C++ ------------------------------------------------------------------------------------------------------------------
def test_cpp_set_skins_and_update_skinned(tmp_path):
    """SampleRenderer::setSkins / updateSkinned of include/SimplePathtracer.h: the hashes of the frame and of the vertex bytes
    the program prints are those of the same skin and pose through the python wrapper."""
    exe = build_dropin(tmp_path, "skin_gpu_test")
    res = run_dropin(exe)
    got = re.search(r"frame ([0-9a-f]{16}) vertices ([0-9a-f]{16})", res.stdout)
    assert got and res.stdout.rstrip().endswith("ok"), res.stdout

    def fnv1a(b):
        h = 1469598103934665603
        for x in b:
            h = ((h ^ x) * 1099511628211) & 0xffffffffffffffff
        return "%016x" % h

    r = dropin_renderer(red_half=(1, 2, 0.5))
    model = r.model
    v = model.meshes[1].vertex
    up = v[:, 1] > 0.5
    j, w = np.zeros((len(v), 4), np.uint16), np.zeros((len(v), 4), F)
    j[up, 1] = 1
    w[up, 0], w[up, 1], w[~up, 0] = 0.25, 0.75, 1.0
    pal = F([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], [0, 0.25, 1, 0.75, 0, 1, 0, 0.25, -1, 0, 0, -0.5]]).reshape(2, 3, 4)
    r.set_skins({1: (j, w)})
    r.update_skinned({1: pal})
    _, px, _ = render(r)
    verts = scene_vertices(r)
    assert np.array_equal(bits(verts), bits(all_vertices(model, {1: sk.apply(v, j, w, pal)})))
    assert (fnv1a(px.tobytes()), fnv1a(verts.tobytes())) == got.groups()
    r.close()
