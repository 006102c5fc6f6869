"""fovpt_set_morphs and fovpt_update_morphed on the GPU: positions and hierarchy bytes against tests/morph_ref.py fed to
fovpt_update_vertices on the same context, frames against the CPU oracle and a fresh build of the moved model, the zero pose,
morph and skin together, absolute semantics, device weights and matrices, ordering with frames in flight, rebuild and the cost
counters, fovpt_temporal_motion's tracking, the life cycle of a mesh's morphs, rejections, a seeded sweep, and the C++ drop-in.
FOVPT_FUZZMO_TO widens the sweep."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import morph_ref as mr
import skin_ref as sk
import temporal_ref as tr
import transform_ref as tf
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer, scenes

import anim_cases as ac
from anim_cases import EMPTY, cornell_morphs, cornell_weights, shaped_targets
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
SEEDS = range(0, int(os.environ.get("FOVPT_FUZZMO_TO", "8")))


# ---- helpers --------------------------------------------------------------------------------------------------------------
def coverage(targets, n):
    """Per vertex, the number of targets that list it."""
    cnt = np.zeros(n, np.int64)
    for t in targets:
        cnt[mr.split(t, n)[0]] += 1
    return cnt


def atrium_morphs(model, big=None, seed=0):
    """Every mesh morphed, target counts cycling 1, 2, 5 and 17; mesh `big` has FOVPT_MORPH_MAX_TARGETS targets."""
    rng = np.random.default_rng(100 + seed)
    return {k: shaped_targets(rng, m.vertex.shape[0], mr.MAX_TARGETS if k == big else (1, 2, 5, 17)[k % 4], 0.5) for k, m in enumerate(model.meshes)}


def atrium_weights(morphs, seed=0):
    rng = np.random.default_rng(200 + seed)
    out = {k: mr.random_weights(rng, len(ts), 0.5) for k, ts in morphs.items()}
    for k, w in out.items():
        if k % 7 and not w.any():
            w[0] = F(0.75)                                                # (most meshes move; every seventh may get a zero pose)
    return out


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
    morphs, w = cornell_morphs(model), cornell_weights()
    r.set_morphs(morphs)
    r.update_morphed(w)
    got = scene_vertices(r)
    want = all_vertices(model, mr.restate(model, morphs, w))
    assert np.array_equal(bits(got), bits(want))
    first = np.cumsum([0] + [m.vertex.shape[0] for m in model.meshes])
    for k in (0, 1, 2, 5):                                                # the meshes not named keep their bits
        assert np.array_equal(bits(got[first[k]:first[k + 1]]), bits(model.meshes[k].vertex))
    for k in (3, 4):
        assert not np.array_equal(got[first[k]:first[k + 1]], model.meshes[k].vertex)
    r.update_morphed({4: w[4]})                                           # one of the two: the other keeps what it last had
    assert np.array_equal(bits(scene_vertices(r)), bits(want))
    r.close()


# ---- 2. batches -----------------------------------------------------------------------------------------------------------
def test_atrium_positions_over_four_batches():
    model = scenes.atrium(8000)
    assert len(model.meshes) == 103                                       # three batches of 32 and a remainder of 7
    nv = [m.vertex.shape[0] for m in model.meshes]
    assert len(set(nv)) > 3 and min(nv) <= 8 and any(n % 256 for n in nv)  # varying max_n, tiny meshes, no multiple of the block
    big = int(np.argmax(nv))
    morphs = atrium_morphs(model, big)
    assert sorted({len(t) for t in morphs.values()}) == [1, 2, 5, 17, mr.MAX_TARGETS]
    cov = {k: coverage(ts, nv[k]) for k, ts in morphs.items()}
    assert any((c == 0).any() for c in cov.values()) and any((c == 1).any() for c in cov.values())     # vertices with 0 and 1 targets
    assert any((c == len(morphs[k])).any() for k, c in cov.items() if len(morphs[k]) > 1)               # ... and with all of them
    assert all(c[-1] > 0 for k, c in cov.items() if len(morphs[k]) % 2 == 0)                             # the last vertex has entries
    assert any(len(mr.split(t, nv[k])[0]) == 0 for k, ts in morphs.items() for t in ts)                  # a target with count 0
    w = atrium_weights(morphs)
    w[big][-1] = F(-1.5)                                                  # the last of the 256 targets is active
    assert any(not x.any() for x in w.values()) and sum(x.any() for x in w.values()) > 80
    r = renderer.SampleRenderer(model)
    r.set_morphs(morphs)
    r.update_morphed(w)
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, mr.restate(model, morphs, w))))
    r.close()


def test_a_mesh_of_several_blocks_and_two_grid_strides():
    """The atrium's meshes have at most 169 vertices: one block each.  A sheet of 520 x 506 = 263120 vertices takes 1024 blocks
    of 256 and 976 vertices of a second stride, beside a sheet of 27 x 26 = 702 (three blocks, the last partly filled) and a mesh
    of 4.  Only a coarse grid of the large sheet's vertices carries triangles: the positions are what is checked."""
    def sheet(nu, nv, step):
        u, v = np.meshgrid(np.arange(nu, dtype=F), np.arange(nv, dtype=F), indexing="ij")
        p = np.stack([u * F(0.5), v * F(0.75), np.sin(u * F(0.4)) + F(0.25) * v], axis=-1).reshape(-1, 3).astype(F)
        q = (np.arange(0, nu - step, step)[:, None] * nv + np.arange(0, nv - step, step)[None, :]).reshape(-1)
        idx = np.concatenate([np.stack([q, q + step * nv, q + step * nv + step], axis=1), np.stack([q, q + step * nv + step, q + step], axis=1)])
        return p, idx.astype(np.uint32)

    floor = scenes.cornell_box().meshes[1]
    meshes = [floor]
    for nu, nv, step in ((520, 506, 8), (27, 26, 1)):
        p, idx = sheet(nu, nv, step)
        meshes.append(scenes.TriangleMesh(p, idx, floor.material, np.zeros((len(p), 2), F), -1))
    model = scenes.Model(meshes)
    n1, n2 = len(meshes[1].vertex), len(meshes[2].vertex)
    assert n1 == 263120 and n1 > 1024 * 256 and n2 == 702 and n2 > 2 * 256 and n2 % 256
    rng = np.random.default_rng(4)
    tail = np.arange(1024 * 256 - 300, n1, 7)
    tail = np.union1d(tail, [n1 - 1]).astype(np.uint32)                   # across the stride's end, up to the last vertex
    wave = np.zeros((n1, 3), F)
    wave[:, 1] = np.cos(meshes[1].vertex[:, 0] * F(0.05))
    morphs = {1: [wave, (tail, rng.uniform(-2, 2, (len(tail), 3)).astype(F)), (np.arange(0, n1, 1000, dtype=np.uint32), rng.uniform(-2, 2, (264, 3)).astype(F))],
              2: shaped_targets(rng, n2, 6), 0: shaped_targets(rng, 4, 2)}
    w = {1: F([0.5, 2.0, -1.0]), 2: F([1.0, -0.5, 3.0, 0.0, 0.25, 1.5]), 0: F([0.0, 1.0])}
    r = renderer.SampleRenderer(model)
    r.set_morphs(morphs)
    r.update_morphed(w)
    got, want = scene_vertices(r), all_vertices(model, mr.restate(model, morphs, w))
    assert np.array_equal(bits(got), bits(want))
    assert not np.array_equal(got[4 + 1024 * 256:4 + n1], meshes[1].vertex[1024 * 256:])      # the second stride moved
    r.close()


# ---- 3. hierarchy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cornell", "atrium"])
def test_hierarchy_is_update_vertices_of_the_restatement(case):
    """On one context (two builds of one model may order their nodes differently): fovpt_update_vertices with the restated
    positions, back to the original ones, then the pose; the same with FOVPT_UPDATE_REBUILD on both sides."""
    model = scenes.atrium(8000) if case == "atrium" else scenes.cornell_box()
    if case == "atrium":
        morphs = atrium_morphs(model, None, 1)
        w = atrium_weights(morphs, 1)
    else:
        morphs, w = cornell_morphs(model), cornell_weights()
    r = renderer.SampleRenderer(model)
    r.set_morphs(morphs)
    h0 = hierarchy(r)
    new = mr.restate(model, morphs, w)
    r.update_vertices(new)
    want = hierarchy(r)
    r.update_vertices(rest_of(model))
    assert same(hierarchy(r), h0)
    r.update_morphed(w)
    assert same(hierarchy(r), want) and not same(want, h0)
    # FOVPT_UPDATE_REBUILD on both sides.  A rebuild of a larger scene does not repeat its own node order (the note above), so the
    # reference is rebuilt twice: where its two hierarchies are the same bytes, the pose's must be those bytes; where they are
    # not, the triangle records -- v0, e1, e2, primitive and mesh, what the leaves hold -- must be the same set of rows.
    rebuilt = []
    for _ in range(2):
        r.update_vertices(rest_of(model), rebuild=True)
        r.update_vertices(new, rebuild=True)
        rebuilt.append(hierarchy(r))
    r.update_vertices(rest_of(model), rebuild=True)
    r.update_morphed(w, rebuild=True)
    got = hierarchy(r)
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, new)))

    def rows(h):
        return h[1][np.lexsort(h[1].T[::-1])]

    assert np.array_equal(rows(rebuilt[0]), rows(rebuilt[1])) and np.array_equal(rows(got), rows(rebuilt[0]))
    if same(rebuilt[0], rebuilt[1]):
        assert same(got, rebuilt[0])
    r.close()


# ---- 4. frames ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["foveated", "fov_off"])
def test_cornell_frames_after_a_pose(oracle, mode):
    size = (96, 64)
    cfg = cfg_uniform(2) if mode == "fov_off" else cfg_foveated(10, 24, (1, 2, 4))
    base = scenes.cornell_box()
    morphs, w = cornell_morphs(base), cornell_weights()
    r = make_gpu(base, PROBE, CORNELL, size, cfg)
    acc0, px0, _ = render(r)
    r.set_morphs(morphs)
    acc1, px1, _ = render(r)                                              # targets alone move nothing
    assert np.array_equal(bits(acc0), bits(acc1)) and np.array_equal(px0, px1)
    r.update_morphed(w)
    cur = moved(base, mr.restate(base, morphs, w))
    acc, px = assert_frame_is_oracle(oracle, r, cur, CORNELL, size, cfg)
    fresh = make_gpu(cur, PROBE, CORNELL, size, cfg)
    facc, fpx, fst = render(fresh)
    st = r.stats()
    assert np.array_equal(bits(acc), bits(facc)) and np.array_equal(px, fpx)
    assert (st.paths, st.radiance_rays, st.shadow_rays) == (fst.paths, fst.radiance_rays, fst.shadow_rays)
    assert not np.array_equal(px, px0)
    fresh.close()
    r.close()


# ---- 5. the zero pose -------------------------------------------------------------------------------------------------------
def test_a_pose_of_zeros_gives_the_rest_bytes():
    """Also a coordinate of -0: the Cornell box's zeros are turned into -0 on the two blocks, which an identity transform turns
    into +0 (test_morph_cpu.py)."""
    base = scenes.cornell_box()
    new = {}
    for k in (3, 4):
        v = base.meshes[k].vertex.copy()
        v[v == 0] = F(-0.0)
        new[k] = v
    model = moved(base, new)
    rest = all_vertices(model)
    assert np.signbit(rest[rest == 0]).any()
    morphs = cornell_morphs(model)
    r = renderer.SampleRenderer(model)
    h0 = hierarchy(r)
    r.set_morphs(morphs)
    r.update_morphed(cornell_weights())
    assert not np.array_equal(bits(scene_vertices(r)), bits(rest))
    r.update_morphed({4: F([0.0, -0.0, 0.0, -0.0]), 3: F([-0.0])})
    assert np.array_equal(bits(scene_vertices(r)), bits(rest)) and same(hierarchy(r), h0)
    r.update_transforms({4: tf.IDENTITY})
    assert not np.array_equal(bits(scene_vertices(r)), bits(rest))       # (what the skip is for)
    r.close()


# ---- 6. morph and skin ------------------------------------------------------------------------------------------------------
def skinned_cornell(model):
    return {4: sk.bend(model.meshes[4].vertex, 3), 3: sk.bend(model.meshes[3].vertex, 1)}


def cornell_palettes(model, k=1.0):
    return {4: sk.bend_pose(model.meshes[4].vertex, 3, 50.0 * k, (-45.0 * k, 0.0, -30.0 * k)),
            3: tf.scale_about((186.0, 0.0, 168.0), (1.0 + 0.3 * k, 1.0 - 0.4 * k, 1.0 - 0.1 * k))[None]}


def test_zero_weights_and_matrices_are_update_skinned():
    model = scenes.cornell_box()
    skins, pal, morphs = skinned_cornell(model), cornell_palettes(model), cornell_morphs(model)
    r = renderer.SampleRenderer(model)
    r.set_skins(skins)
    r.set_morphs(morphs)
    r.update_skinned(pal)
    want_v, want_h = scene_vertices(r), hierarchy(r)
    r.update_vertices(rest_of(model))
    assert not same(hierarchy(r), want_h)
    r.update_morphed({k: (np.zeros(len(morphs[k]), F), pal[k]) for k in (3, 4)})
    assert np.array_equal(bits(scene_vertices(r)), bits(want_v)) and same(hierarchy(r), want_h)
    # fovpt_update_skinned of a morphed mesh is what it was: rest through the skin
    r.update_morphed({k: (cornell_weights()[k], pal[k]) for k in (3, 4)})
    assert not np.array_equal(bits(scene_vertices(r)), bits(want_v))
    r.update_skinned(pal)
    assert np.array_equal(bits(scene_vertices(r)), bits(want_v)) and same(hierarchy(r), want_h)
    r.close()


def test_morph_and_skin_together_are_the_restatement_composed():
    """Every mesh of the atrium morphed and skinned; two poses in three carry a palette, so that both kernels run in one call and
    their batches fill at different times."""
    model = scenes.atrium(8000)
    morphs = atrium_morphs(model, None, 2)
    w = atrium_weights(morphs, 2)
    skins = {k: sk.bend(m.vertex, (1, 2, 5, 17)[(k + 1) % 4]) for k, m in enumerate(model.meshes)}
    rng = np.random.default_rng(6)
    pal = {k: sk.bend_pose(model.meshes[k].vertex, s[2], 3.0 * k + 1.0, rng.uniform(-6.0, 6.0, 3)) for k, s in skins.items()}
    poses = {k: ((w[k], pal[k]) if k % 3 else w[k]) for k in morphs}
    assert sum(isinstance(p, tuple) for p in poses.values()) > 64 and sum(not isinstance(p, tuple) for p in poses.values()) > 32
    for k, p in poses.items():
        assert mr.accepted(model.meshes[k].vertex, morphs[k], w[k], *((skins[k][1], pal[k]) if k % 3 else ()))
    r = renderer.SampleRenderer(model)
    r.set_morphs(morphs)
    r.set_skins(skins)
    new = mr.restate(model, morphs, poses, skins)
    r.update_vertices(new)
    want_h = hierarchy(r)
    r.update_vertices(rest_of(model))
    r.update_morphed(poses)
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, new))) and same(hierarchy(r), want_h)
    skinned_only = sk.restate(model, skins, {k: pal[k] for k in (1, 2)})
    for k in (1, 2):
        if w[k].any():
            assert not np.array_equal(bits(new[k]), bits(skinned_only[k]))                 # (the morph shows through the skin)
    r.close()


# ---- 7. absolute ------------------------------------------------------------------------------------------------------------
def test_poses_are_absolute_and_start_from_rest():
    model = scenes.cornell_box()
    morphs, w1, w2 = cornell_morphs(model), cornell_weights(1.0), cornell_weights(0.4)
    r = renderer.SampleRenderer(model)
    r.set_morphs(morphs)
    r.update_vertices(mr.restate(model, morphs, w2))
    want = hierarchy(r)
    want_v = all_vertices(model, mr.restate(model, morphs, w2))
    r.update_vertices(rest_of(model))
    r.update_morphed(w1)
    r.update_morphed(w2)                                                  # W2 of rest, not W2 of W1 of rest
    assert same(hierarchy(r), want) and np.array_equal(bits(scene_vertices(r)), bits(want_v))
    # a mesh fovpt_update_vertices has deformed is set from the fovpt_set_scene positions again; another deformed mesh stays
    j2, j4 = jitter(model.meshes[2].vertex, 3, 9.0), jitter(model.meshes[4].vertex, 4, 9.0)
    r.update_vertices({2: j2, 4: j4})
    r.update_morphed(w2)
    new = mr.restate(model, morphs, w2)
    new[2] = j2
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, new)))
    r.update_vertices({2: model.meshes[2].vertex})
    assert same(hierarchy(r), want)
    # a pose, then fovpt_update_transforms on the same (still morphed) mesh: the transform of rest alone
    m = sk.dense_matrix()
    r.update_transforms({4: m})
    new = mr.restate(model, morphs, w2)
    new[4] = tf.apply(model.meshes[4].vertex, m)
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, new)))
    r.update_morphed({4: w1[4]})                                          # ... and back under the targets, from rest
    new[4] = mr.apply(model.meshes[4].vertex, morphs[4], w1[4])
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, new)))
    r.close()


# ---- 8. device data ---------------------------------------------------------------------------------------------------------
def test_device_weights_and_matrices_give_the_host_bytes():
    import torch
    model = scenes.atrium(8000)
    morphs = atrium_morphs(model, None, 3)
    w = atrium_weights(morphs, 3)
    skins = {k: sk.bend(m.vertex, 1 + k % 5) for k, m in enumerate(model.meshes) if k % 2}
    pal = {k: sk.bend_pose(model.meshes[k].vertex, s[2], 2.0 * k + 1.0, (0.5, 0.0, -0.25)) for k, s in skins.items()}
    poses = {k: ((w[k], pal[k]) if k in skins else w[k]) for k in morphs}
    r = renderer.SampleRenderer(model)
    r.set_morphs(morphs)
    r.set_skins(skins)
    r.update_morphed(poses)
    want_v, want_h = scene_vertices(r), hierarchy(r)
    assert np.array_equal(bits(want_v), bits(all_vertices(model, mr.restate(model, morphs, poses, skins))))
    r.update_vertices(rest_of(model))
    assert not same(hierarchy(r), want_h)
    dw = {k: torch.from_numpy(x).cuda() for k, x in w.items()}
    dp = {k: torch.from_numpy(np.ascontiguousarray(p, F)).cuda() for k, p in pal.items()}
    torch.cuda.synchronize()
    dev = {k: ((dw[k], dp[k]) if k in skins else dw[k]) for k in morphs}
    r.update_morphed(dev)
    assert np.array_equal(bits(scene_vertices(r)), bits(want_v)) and same(hierarchy(r), want_h)
    with pytest.raises(ValueError):
        r.update_morphed({0: w[0], 1: dev[1]})
    with pytest.raises(ValueError):
        r.update_morphed({1: (dw[1], pal[1])})
    with pytest.raises(ValueError):
        r.update_morphed({0: dw[0].reshape(1, -1)})
    r.close()


# ---- 9. frames in flight ------------------------------------------------------------------------------------------------------
def test_poses_between_frames_in_flight(oracle):
    import torch
    size = (96, 64)
    cfg = cfg_foveated(10, 24, (1, 2, 4))
    cfg.frames_in_flight = 2
    base = scenes.cornell_box()
    morphs = cornell_morphs(base)
    poses = [cornell_weights(k) for k in (0.3, 0.65, 1.0)]
    shape = (size[1], size[0])
    r = make_gpu(base, PROBE, CORNELL, size, cfg)
    r.set_morphs(morphs)
    outs = [(torch.zeros(shape + (4,), dtype=torch.float32, device="cuda"), torch.zeros(shape, dtype=torch.int32, device="cuda")) for _ in poses]
    torch.cuda.synchronize()
    for p, b in zip(poses, outs):                                         # pose, frame, pose, frame, pose, frame: no synchronisation
        r.update_morphed(p)
        f = r.launchParams.frame
        f.accum_buffer, f.frame_buffer = b[0].data_ptr(), b[1].data_ptr()
        f.subframe_index = 0
        r.render_async()
    r.synchronize()
    frames = []
    for k, (p, b) in enumerate(zip(poses, outs)):
        Fr, _ = oracle_frame(oracle, moved(base, mr.restate(base, morphs, p)), CORNELL, size, cfg)
        acc, px = b[0].cpu().numpy(), b[1].cpu().numpy()
        assert np.array_equal(bits(acc), bits(Fr.accum)) and np.array_equal(px.view(np.uint32), Fr.frame), "pose %d" % k
        frames.append(px)
    assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[1], frames[2])
    r.close()


# ---- 10. rebuild ----------------------------------------------------------------------------------------------------------
def test_rebuild_and_the_cost_counters():
    base = scenes.cornell_box()
    size, cfg = (96, 64), cfg_foveated(10, 24, (1, 2, 4))
    morphs, w = cornell_morphs(base), cornell_weights()
    r = make_gpu(base, PROBE, CORNELL, size, cfg)
    trav = r.launchParams.traversable
    r.set_morphs(morphs)
    assert r.hierarchy_cost().updates == 0                                # targets are no update
    r.update_morphed(w)
    c1 = r.hierarchy_cost(wait=True)
    assert (c1.updates, c1.measured) == (1, 1)                            # a refit pose is counted ...
    refit = render(r)
    r.update_morphed(w, rebuild=True)
    c2 = r.hierarchy_cost()
    assert (c2.updates, c2.measured) == (2, 2) and c2.current == c2.built  # ... and so is a rebuild, which measures at once
    assert r.launchParams.traversable == trav
    rebuilt = render(r)
    assert np.array_equal(bits(refit[0]), bits(rebuilt[0])) and np.array_equal(refit[1], rebuilt[1])
    fresh = make_gpu(moved(base, mr.restate(base, morphs, w)), PROBE, CORNELL, size, cfg)
    want = render(fresh)
    assert np.array_equal(bits(rebuilt[0]), bits(want[0])) and np.array_equal(rebuilt[1], want[1])
    r.update_morphed({}, rebuild=True)                                    # a rebuild alone
    assert r.hierarchy_cost().updates == 3
    r.update_morphed({})                                                  # nothing to do: not counted
    assert r.hierarchy_cost().updates == 3
    r.update_morphed(cornell_weights(0.5))
    c3 = r.hierarchy_cost(wait=True)
    assert (c3.updates, c3.measured) == (4, 4)
    fresh.close()
    r.close()


# ---- 11. temporal ---------------------------------------------------------------------------------------------------------
def test_temporal_motion_sees_poses_as_vertex_updates():
    size = (192, 120)
    base = scenes.cornell_box()
    morphs, w = cornell_morphs(base), cornell_weights(0.5)
    d = tcfg(CAPS)
    outs = []
    for use_morph in (True, False):
        cfg = cfg_foveated(12, 36, (1, 2, 4))
        cfg.write_guides = 1
        r = make_gpu(base, PROBE, CORNELL, size, cfg)
        r.set_morphs(morphs)
        r.render()
        r.temporal_motion(d, None, None, None, r.motion_buffer())
        if use_morph:
            r.update_morphed(w)
        else:
            r.update_vertices(mr.restate(base, morphs, w))
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


# ---- 12. the life cycle of a mesh's morphs ----------------------------------------------------------------------------------
def test_set_morphs_replaces_removes_and_ends_with_the_scene():
    model = scenes.cornell_box()
    n4 = model.meshes[4].vertex.shape[0]
    r = renderer.SampleRenderer(model)
    morphs, w = cornell_morphs(model), cornell_weights()
    r.set_morphs(morphs)
    r.update_morphed(w)
    # replace mesh 4's targets (another count: mesh 3's places in the arrays move, before it in mesh order or not); mesh 3's stay
    rng = np.random.default_rng(3)
    new4 = shaped_targets(rng, n4, 7, 25.0)
    r.set_morphs({4: new4})
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, mr.restate(model, morphs, w))))     # geometry does not move
    morphs[4] = new4
    w[4] = mr.random_weights(rng, 7, 0.7)
    r.update_morphed(w)
    want = all_vertices(model, mr.restate(model, morphs, w))
    assert np.array_equal(bits(scene_vertices(r)), bits(want))
    old = np.ascontiguousarray(cornell_weights()[4])
    ps = (abi.MorphPose * 1)()
    ps[0].mesh, ps[0].num_targets, ps[0].weights = 4, 4, old.ctypes.data
    assert r._L.fovpt_update_morphed(r._ctx, ps, 1, 0) == E_INVALID       # the old target count
    # fovpt_set_skins afterwards leaves the morphs alone
    r.set_skins({4: sk.bend(model.meshes[4].vertex, 2), 0: sk.bend(model.meshes[0].vertex, 3)})
    assert np.array_equal(bits(scene_vertices(r)), bits(want))
    r.update_morphed(w)
    assert np.array_equal(bits(scene_vertices(r)), bits(want))
    r.set_skins({4: None, 0: None})
    r.update_morphed({3: w[3]})
    assert np.array_equal(bits(scene_vertices(r)), bits(want))
    # remove mesh 3's targets: a pose for it is refused, mesh 4 still poses
    h = hierarchy(r)
    r.set_morphs({3: None})
    with pytest.raises(lib.FovptError):
        r.update_morphed({3: w[3]})
    with pytest.raises(lib.FovptError):
        r.update_morphed(w)                                               # ... also beside a good one: all or nothing
    assert np.array_equal(bits(scene_vertices(r)), bits(want)) and same(hierarchy(r), h)
    w4 = {4: mr.random_weights(rng, 7, 0.7)}
    r.update_morphed(w4)
    new = mr.restate(model, morphs, w)
    new[4] = mr.restate(model, morphs, w4)[4]
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, new)))
    r.set_morphs({4: None})                                               # the last morphed mesh goes
    with pytest.raises(lib.FovptError):
        r.update_morphed(w4)
    r.set_morphs({4: new4})
    # fovpt_set_scene drops every mesh's targets
    md, n, td, nt, keep = scenes.pack_model(model)
    trav = C.c_uint64()
    r._check(r._L.fovpt_set_scene(r._ctx, C.cast(md, C.c_void_p), n, C.cast(td, C.c_void_p), nt, C.byref(trav)))
    for k in (3, 4):
        with pytest.raises(lib.FovptError):
            r.update_morphed({k: w[k]})
    r.set_morphs({4: new4})                                               # and a new scene takes new ones
    r.update_morphed(w4)
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, mr.restate(model, morphs, w4))))
    r.close()


# ---- 13. rejections -------------------------------------------------------------------------------------------------------
def test_rejections_change_nothing():
    base = scenes.cornell_box()
    r = renderer.SampleRenderer(base)
    L = r._L
    n4 = base.meshes[4].vertex.shape[0]
    morphs, skins = ac.morph_scene(base)                                  # D = 2^100 on mesh 5, S = 4 on mesh 3
    r.set_morphs(morphs)
    r.set_skins(skins)
    w = cornell_weights()
    r.update_morphed(w)
    before_v, before_h = scene_vertices(r), hierarchy(r)

    def unchanged():
        return np.array_equal(bits(scene_vertices(r)), bits(before_v)) and same(hierarchy(r), before_h)

    # -- fovpt_set_morphs
    idx = np.arange(0, n4, 2, dtype=np.uint32)
    delta = np.ones((len(idx), 3), F)
    for what, entries, n in ac.morph_set_cases(base):
        packed, keep = ac.pack_morphs(entries)
        assert L.fovpt_set_morphs(r._ctx, packed, len(entries) if n is None else n) == E_INVALID, what
        ac.assert_recorded("morphs", what, E_INVALID, L.fovpt_last_error(r._ctx))
        assert unchanged(), what
    assert L.fovpt_set_morphs(r._ctx, None, 1) == E_INVALID
    assert L.fovpt_set_morphs(None, None, 0) == E_INVALID
    assert L.fovpt_set_morphs(r._ctx, None, 0) == 0                       # nothing to do
    for bad in ([np.zeros((n4, 2), F)], [np.zeros((n4 - 1, 3), F)], [(idx, delta[:-1])], [(idx.astype(F), delta)], [(idx.reshape(1, -1), delta)], []):
        with pytest.raises(ValueError):                                   # the wrapper's own checks
            r.set_morphs({4: bad})
    r.update_morphed(w)                                                   # the targets are the ones set before the refused calls
    assert unchanged()

    # -- fovpt_update_morphed
    W4, W3 = np.ascontiguousarray(cornell_weights(0.5)[4]), np.ascontiguousarray(w[3])      # (a good entry would move the block)
    P4, P3 = np.ascontiguousarray(sk.bend_pose(base.meshes[4].vertex, 3, 20.0, (1.0, 2.0, 3.0))), np.ascontiguousarray(tf.IDENTITY[None])

    def pose(mesh=4, nt=4, wts=W4, nj=0, reserved=0, m=None):
        return dict(mesh=mesh, nt=nt, weights=wts, nj=nj, reserved=reserved, m=m)

    def update(entries, n=None, flags=0, ctx=r._ctx):
        return L.fovpt_update_morphed(ctx, ac.pack_morph_poses(entries), len(entries) if n is None else n, flags)

    row_only = ac.row_only
    for what, entries, n, flags, _ in ac.morph_pose_cases(base, morphs, w):
        assert update(entries, n, flags) == E_INVALID, (what, n, flags)
        ac.assert_recorded("morphed", what, E_INVALID, L.fovpt_last_error(r._ctx))
        assert unchanged(), what
    assert L.fovpt_update_morphed(r._ctx, None, 1, 0) == E_INVALID
    assert L.fovpt_update_morphed(None, None, 0, 0) == E_INVALID
    assert L.fovpt_update_morphed(r._ctx, None, 0, 0) == 0                # nothing to do
    assert unchanged()
    assert r.hierarchy_cost(wait=True).updates == 2                       # the two accepted calls, none of the refused ones
    for bad in (np.zeros((2, 2), F), (W4, np.zeros((3, 3, 3), F)), (W4, np.tile(np.diag(F([1, 1, 1, 2])), (3, 1, 1)))):      # the wrapper's own checks
        with pytest.raises(ValueError):
            r.update_morphed({4: bad})
    r.update_morphed({4: (w[4], np.tile(np.eye(4, dtype=F), (3, 1, 1)))})  # the (J, 4, 4) form
    r.update_morphed({4: w[4]})
    assert unchanged()
    # -- exactly 2^127 is not above: accepted, finite, and the restatement's.  Mesh 5 with w = 2^27 has B = 2^127 as the rule
    #    computes it, in binary64; the row rule is met exactly on mesh 3.
    cur = mr.restate(base, morphs, w)
    w5 = F([2.0 ** 27])
    assert mr.bound(base.meshes[5].vertex, morphs[5], w5) == 2.0 ** 127 and mr.accepted(base.meshes[5].vertex, morphs[5], w5)
    assert update([pose(mesh=5, nt=1, wts=w5)]) == 0
    cur[5] = mr.apply(base.meshes[5].vertex, morphs[5], w5)
    m3 = row_only(F(2.0 ** 125))
    assert mr.row_bound(base.meshes[3].vertex, morphs[3], w[3], skins[3][1], m3) == 2.0 ** 127
    assert mr.accepted(base.meshes[3].vertex, morphs[3], w[3], skins[3][1], m3)
    assert update([pose(mesh=3, nt=1, wts=W3, nj=1, m=m3)]) == 0
    cur[3] = mr.apply_skinned(base.meshes[3].vertex, morphs[3], w[3], skins[3][0], skins[3][1], m3)
    got = scene_vertices(r)
    assert np.isfinite(got).all() and (got == F(2.0 ** 127)).any()
    assert np.array_equal(bits(got), bits(all_vertices(base, cur)))
    r.close()
    ctx = C.c_void_p()                                                    # no scene
    lib.check(None, L.fovpt_create(C.byref(ctx), 0))
    assert L.fovpt_set_morphs(ctx, None, 0) == E_NO_SCENE
    assert L.fovpt_update_morphed(ctx, None, 0, 0) == E_NO_SCENE
    L.fovpt_destroy(ctx)


def test_more_than_2_to_the_32_entries_are_refused():
    """The size at which the count can go wrong: one mesh of 2^24 vertices (one triangle) with 256 dense targets, which share one
    array of deltas, has 2^32 entries, one more than fit.  The count is checked before the deltas are read, so the refusal
    costs nothing of that size."""
    n = 1 << 24
    v = np.zeros((n, 3), F)
    v[:3] = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    floor = scenes.cornell_box().meshes[1]
    model = scenes.Model([floor, scenes.TriangleMesh(v, np.array([[0, 1, 2]], np.uint32), floor.material, np.zeros((n, 2), F), -1)])
    r = renderer.SampleRenderer(model)
    delta = np.zeros((n, 3), F)
    ts = (abi.MorphTarget * 256)()
    for t in range(256):
        ts[t].count, ts[t].delta = n, delta.ctypes.data
    mm = (abi.MeshMorph * 1)()
    mm[0].mesh, mm[0].num_vertices, mm[0].num_targets, mm[0].targets = 1, n, 256, ts
    assert r._L.fovpt_set_morphs(r._ctx, mm, 1) == E_INVALID
    r.set_morphs({0: [np.ones((4, 3), F)]})                               # nothing was kept of it: another mesh still takes targets
    r.update_morphed({0: F([1.0])})
    assert np.array_equal(bits(scene_vertices(r)[:4]), bits(floor.vertex + F(1.0)))
    r.close()


# ---- 14. a seeded sweep -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep_scene():
    model = scenes.atrium(2000)
    r = renderer.SampleRenderer(model)
    rng = np.random.default_rng(77)
    skins = {k: sk.random_skin(rng, m.vertex.shape[0], 1 + k % 6) for k, m in enumerate(model.meshes) if k % 3 == 0}
    r.set_skins(skins)
    yield model, r, hierarchy(r), skins
    r.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_targets_and_weights(sweep_scene, seed):
    model, r, h0, skins = sweep_scene
    nmesh = len(model.meshes)
    assert nmesh > 32 and nmesh % 32 != 0
    rng = np.random.default_rng(3000 + seed)
    named = [k for k in range(nmesh) if rng.uniform() < (1.0 if seed % 4 == 0 else 0.6)]      # every fourth seed: all of them
    morphs = {k: mr.random_targets(rng, model.meshes[k].vertex.shape[0], int(rng.integers(1, 13)), dense=int(rng.integers(0, 3)),
                                   fraction=float(rng.uniform(0.02, 0.6)), scale=0.5) for k in named}
    r.set_morphs({k: morphs.get(k) for k in range(nmesh)})                # (the others lose what an earlier seed gave them)
    posed = [k for k in named if rng.uniform() < 0.8] or named[:1]
    poses = {}
    for k in posed:
        w = mr.random_weights(rng, len(morphs[k]), float(rng.uniform(0.2, 1.0)))
        if k in skins and rng.uniform() < 0.7:
            poses[k] = (w, sk.random_pose(rng, model.meshes[k].vertex, skins[k][2]))
        else:
            poses[k] = w
    ws = np.concatenate([p[0] if isinstance(p, tuple) else p for p in poses.values()])
    assert (ws == 0).any() and (ws < 0).any() and (ws > 1).any() and any(isinstance(p, tuple) for p in poses.values())
    for k, p in poses.items():                                            # every drawn case is within the rules: none is skipped
        if isinstance(p, tuple):
            assert mr.accepted(model.meshes[k].vertex, morphs[k], p[0], skins[k][1], p[1]), k
        else:
            assert mr.accepted(model.meshes[k].vertex, morphs[k], p), k
    want_v = mr.restate(model, morphs, poses, skins)
    r.update_vertices(rest_of(model))
    assert same(hierarchy(r), h0)
    r.update_vertices(want_v)
    want_h = hierarchy(r)
    r.update_vertices(rest_of(model))
    r.update_morphed(poses)
    assert np.array_equal(bits(scene_vertices(r)), bits(all_vertices(model, want_v)))
    assert same(hierarchy(r), want_h) and not same(want_h, h0)


# ---- 15. C++ ------------------------------------------------------------------------------------------------------------------
def test_cpp_set_morphs_and_update_morphed(tmp_path):
    """SampleRenderer::setMorphs / updateMorphed of include/SimplePathtracer.h: the hashes of the frame and of the vertex bytes
    the program prints are those of the same targets and weights through the python wrapper."""
    exe = build_dropin(tmp_path, "morph_gpu_test")
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
    lean = np.zeros_like(v)
    lean[:, 0], lean[:, 2] = F(0.25) * v[:, 1], F(-0.125)
    upper = np.flatnonzero(v[:, 1] > 0.5).astype(np.uint32)
    lift = np.zeros((len(upper), 3), F)
    lift[:, 1], lift[:, 2] = 0.5, F(0.0625) * (upper % 3).astype(F)
    targets, w = [lean, (upper, lift), EMPTY], F([1.5, -0.75, 2.0])
    r.set_morphs({1: targets})
    r.update_morphed({1: w})
    _, px, _ = render(r)
    verts = scene_vertices(r)
    assert np.array_equal(bits(verts), bits(all_vertices(model, {1: mr.apply(v, targets, w)})))
    assert (fnv1a(px.tobytes()), fnv1a(verts.tobytes())) == got.groups()
    r.close()
