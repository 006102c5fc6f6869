"""The calls the animation set-up refuses, one list per call, shared by the GPU tests (test_rig_gpu, test_morph_gpu, test_skin_gpu,
test_transform_gpu: test_rejections_change_nothing) and by tests/test_anim_plan_cpu.py, which runs the same cases through
csrc/fovpt_animplan.h without a GPU.  A case is a name and a plain description of the call: counts as the caller states them,
arrays (numpy) or None for a null pointer, reserved fields.  pack_*() turns a description into the ctypes structs of the C ABI;
tests/test_anim_plan_cpu.py serialises it for its driver.  The fixtures the cases are mutations of (the Cornell box with skins,
morph targets and a rig) are here too, so that both sides build them the same way.

tests/golden/anim_rejections.json holds, per list and case name, the code and the text (fovpt_last_error) the library gave
before the rules moved into the header; recorded() is what both sides compare with, pointer values masked."""
import copy
import ctypes as C
import json
import os
import re

import numpy as np

import morph_ref as mr
import rig_ref as rg
import skin_ref as sk
import transform_ref as tf
from fovpathtracing_optixcodelatest_amd import abi

F = np.float32
E_INVALID = -1
TALL, SHORT = 4, 3
EMPTY = (np.zeros(0, np.uint32), np.zeros((0, 3), F))
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anim_rejections.json")
nan, inf = np.nan, np.inf


def masked(text):
    """An error text with the values of %p replaced."""
    if isinstance(text, bytes):
        text = text.decode("utf-8", "replace")
    return re.sub(r"0x[0-9a-fA-F]+|\(nil\)", "PTR", text)


_golden = None


def recorded(call, name):
    """(code, text) of case `name` of list `call` in the record."""
    global _golden
    if _golden is None:
        with open(GOLDEN_PATH) as f:
            _golden = json.load(f)
    code, text = _golden[call][name]
    return code, text


def assert_recorded(call, name, code, text):
    """What the GPU tests and the CPU test hold a refusal to: the recorded code and text."""
    assert (code, masked(text)) == recorded(call, name), (call, name, code, masked(text), recorded(call, name))


def names_are_unique(cases):
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return cases


def below(x):
    return np.nextafter(F(x), F(0))


def above(x):
    return np.nextafter(F(x), F(inf))


def with_entry(a, i, v):
    """A copy of an array with one entry, counted over the flattened array, changed."""
    x = np.array(a).copy()
    x.reshape(-1)[i] = v
    return x


def row_only(t):
    """One joint whose first row is 0 0 0 t: the row's bound is S |t| whatever the positions' bound is."""
    m = np.tile(tf.IDENTITY, (1, 1, 1))
    m[0, 0] = (0, 0, 0, t)
    return m


def _ptr(a):
    return None if a is None else a.ctypes.data


# ---- fovpt_set_skins / fovpt_update_skinned -----------------------------------------------------------------------------------------
def cornell_skins(model):
    """The tall block (mesh 4) bends over 3 joints, the short block (3) has one."""
    return {4: sk.bend(model.meshes[4].vertex, 3), 3: sk.bend(model.meshes[3].vertex, 1)}


def cornell_poses(model, k=1.0):
    return {4: sk.bend_pose(model.meshes[4].vertex, 3, 50.0 * k, (-45.0 * k, 0.0, -30.0 * k)),
            3: tf.scale_about((186.0, 0.0, 168.0), (1.0 + 0.3 * k, 1.0 - 0.4 * k, 1.0 - 0.1 * k))[None]}


def skin_scene(base):
    """The skins the rejection tests set first: cornell_skins with S = 4 on mesh 3, and one joint of weight 1 (S = 1) on mesh 5."""
    skins = cornell_skins(base)
    w4 = skins[3][1].copy()
    w4[0] = 1
    skins[3] = (skins[3][0], w4, 1)
    assert sk.weight_sum(skins[3][1]) == 4.0 and abs(sk.weight_sum(skins[4][1]) - 1.0) < 1e-6
    skins[5] = sk.bend(base.meshes[5].vertex, 1)
    assert sk.weight_sum(skins[5][1]) == 1.0
    return skins


def skin_set_cases(base, skins):
    """(name, entries, num): entries of dict(mesh, nv, nj, reserved, joints, weights); num None: as many as there are entries."""
    n3, n4 = base.meshes[3].vertex.shape[0], base.meshes[4].vertex.shape[0]
    j4, wt4 = np.ascontiguousarray(skins[4][0]), np.ascontiguousarray(skins[4][1])
    assert j4.max() == 2

    def skin(mesh=4, nv=n4, nj=3, reserved=0, joints=j4, weights=wt4):
        return dict(mesh=mesh, nv=nv, nj=nj, reserved=reserved, joints=joints, weights=weights)

    zero_slot = int(np.flatnonzero(wt4.reshape(-1) == 0)[0])             # a slot whose weight is 0: its index counts all the same
    return names_are_unique([
        ("num below 0", [skin()], -1),
        ("mesh above", [skin(mesh=6)], None), ("mesh below", [skin(mesh=-1)], None),
        ("listed twice", [skin(), skin()], None),
        ("a vertex fewer", [skin(nv=n4 - 1)], None), ("a vertex more", [skin(nv=n4 + 1)], None),      # num_vertices other than the mesh's
        ("no vertices when removing", [skin(nv=0, nj=0, joints=None, weights=None)], None),
        ("joints above the cap", [skin(nj=sk.MAX_JOINTS + 1)], None),
        ("null joints", [skin(joints=None)], None), ("null weights", [skin(weights=None)], None),
        ("null joints and weights", [skin(joints=None, weights=None)], None),
        ("removing with two pointers", [skin(nj=0)], None), ("removing with one pointer", [skin(nj=0, weights=None)], None),
        ("reserved", [skin(reserved=1)], None),
        ("joint index above", [skin(joints=with_entry(j4, 5, 3))], None),
        ("joint index above where the weight is 0", [skin(joints=with_entry(j4, zero_slot, 3))], None),
        ("fewer joints than the indices use", [skin(nj=2)], None),
        ("weight nan", [skin(weights=with_entry(wt4, 0, nan))], None), ("weight inf", [skin(weights=with_entry(wt4, 7, inf))], None),
        ("weight below 0", [skin(weights=with_entry(wt4, 2, -1e-30))], None),
        ("weight above 1", [skin(weights=with_entry(wt4, 4 * n4 - 1, np.nextafter(F(1), F(2))))], None),
        ("the second skin is bad", [skin(mesh=3, nv=n3, nj=1, joints=skins[3][0], weights=skins[3][1]), skin(weights=with_entry(wt4, 1, 2.0))], None),
    ])


def pack_skins(entries):
    s = (abi.MeshSkin * max(1, len(entries)))()
    for k, e in enumerate(entries):
        s[k].mesh, s[k].num_vertices, s[k].num_joints, s[k]._reserved = e["mesh"], e["nv"], e["nj"], e["reserved"]
        s[k].joints, s[k].weights = _ptr(e["joints"]), _ptr(e["weights"])
    return s


def skin_pose_cases(base, poses):
    """(name, entries, num, flags, rule): entries of dict(mesh, nj, m); rule: whether an overflow rule of the header refuses the
    case (the others are refused by what fovpt_update_skinned checks against its context).  The good entry of mesh 4 is another
    pose than the scene's current one: accepted, it would move the block."""
    P3, P4 = np.ascontiguousarray(poses[3]), np.ascontiguousarray(poses[4])
    other = np.ascontiguousarray(cornell_poses(base, 0.5)[4])
    assert 400 < np.abs(base.meshes[4].vertex).max() < 600

    def pose(mesh=4, nj=3, m=other):
        return dict(mesh=mesh, nj=nj, m=m)

    return names_are_unique([
        ("num below 0", [pose()], -1, 0, False),
        ("mesh above", [pose(mesh=6)], None, 0, False), ("mesh below", [pose(mesh=-1)], None, 0, False),
        ("listed twice", [pose(), pose()], None, 0, False),
        ("a mesh without a skin", [pose(mesh=2)], None, 0, False),
        ("fewer joints than the skin", [pose(nj=2)], None, 0, False), ("more joints than the skin", [pose(nj=4)], None, 0, False),
        ("null matrices", [pose(m=None)], None, 0, False), ("null device matrices", [pose(m=None)], None, abi.UPDATE_DEVICE, False),
        ("flag 4", [pose()], None, 4, False), ("flag 8 with rebuild", [pose()], None, 8 | abi.UPDATE_REBUILD, False),
        ("entry nan", [pose(m=with_entry(P4, 5, nan))], None, 0, True),
        ("entry inf", [pose(m=with_entry(P4, 12, inf))], None, 0, True),
        ("entry -inf with rebuild", [pose(m=with_entry(P4, 35, -inf))], None, abi.UPDATE_REBUILD, True),
        ("row above the bound", [pose(m=with_entry(P4, 2, 1e36))], None, 0, True),      # 1e36 A > 2^127 = 1.7e38 (the block's A is between 400 and 600)
        ("translation above the bound", [pose(m=with_entry(P4, 19, 1.8e38))], None, 0, True),
        ("S 1, an ulp above 2^127", [pose(mesh=5, nj=1, m=row_only(above(2.0 ** 127)))], None, 0, True),
        ("S 4, an ulp above 2^125", [pose(mesh=3, nj=1, m=row_only(above(2.0 ** 125)))], None, 0, True),
        ("the second pose is bad", [pose(), pose(mesh=3, nj=1, m=with_entry(P3, 9, nan))], None, 0, True),      # nothing of the first
    ])


def pack_skin_poses(entries):
    p = (abi.SkinPose * max(1, len(entries)))()
    for k, e in enumerate(entries):
        p[k].mesh, p[k].num_joints, p[k].matrices = e["mesh"], e["nj"], _ptr(e["m"])
    return p


# ---- fovpt_set_morphs / fovpt_update_morphed ----------------------------------------------------------------------------------------
def shaped_targets(rng, n, nt, scale=4.0):
    """nt targets for n vertices with the shapes that can go wrong: target 0 dense when nt is odd; from five targets on, target
    2 is empty; the last target is sparse and lists the mesh's last vertex; the others are sparse over about a third of the
    vertices."""
    ts = mr.random_targets(rng, n, nt, dense=nt % 2, fraction=0.3, scale=scale)
    if nt >= 5:
        ts[2] = EMPTY
    if isinstance(ts[-1], tuple) and n:
        idx = np.union1d(ts[-1][0], [n - 1]).astype(np.uint32)
        ts[-1] = (idx, rng.uniform(-scale, scale, (len(idx), 3)).astype(F))
    return ts


def cornell_morphs(model):
    """The tall block (mesh 4) has four targets (sparse, sparse, sparse, sparse with the last vertex), the short block (3) one
    dense target."""
    rng = np.random.default_rng(17)
    return {4: shaped_targets(rng, model.meshes[4].vertex.shape[0], 4, 40.0), 3: shaped_targets(rng, model.meshes[3].vertex.shape[0], 1, 30.0)}


def cornell_weights(k=1.0):
    return {4: F([0.9 * k, 0.0, -0.6 * k, 1.4 * k]), 3: F([1.25 * k])}


def morph_scene(base):
    """(morphs, skins) the rejection tests set first: cornell_morphs with D = 2^100 on mesh 5 (never posed far: for the bound), the
    tall block's bend and S = 4 on mesh 3."""
    n3, n5 = base.meshes[3].vertex.shape[0], base.meshes[5].vertex.shape[0]
    morphs = cornell_morphs(base)
    morphs[5] = [np.full((n5, 3), 2.0 ** 100, F)]
    skins = {4: sk.bend(base.meshes[4].vertex, 3), 3: (np.zeros((n3, 4), np.uint16), np.ones((n3, 4), F), 1)}
    return morphs, skins


def morph_set_cases(base):
    """(name, entries, num): entries of dict(mesh, nv, nt, reserved, targets), targets None or a list of dict(count, reserved,
    index, delta)."""
    n3, n4 = base.meshes[3].vertex.shape[0], base.meshes[4].vertex.shape[0]
    idx = np.arange(0, n4, 2, dtype=np.uint32)
    delta = np.ones((len(idx), 3), F)
    dense = np.ones((n4, 3), F)

    def target(count=len(idx), reserved=0, index=idx, d=delta):
        return dict(count=count, reserved=reserved, index=index, delta=d)

    def morph(mesh=4, nv=n4, nt=None, reserved=0, targets=(target(),), null_targets=False):
        return dict(mesh=mesh, nv=nv, nt=len(targets) if nt is None else nt, reserved=reserved, targets=None if null_targets else list(targets))

    return names_are_unique([
        ("num below 0", [morph()], -1),
        ("mesh above", [morph(mesh=6)], None), ("mesh below", [morph(mesh=-1)], None),
        ("listed twice", [morph(), morph()], None),
        ("a vertex fewer", [morph(nv=n4 - 1)], None), ("a vertex more", [morph(nv=n4 + 1)], None),
        ("no vertices when removing", [morph(nv=0, nt=0, null_targets=True)], None),
        ("targets above the cap", [morph(nt=mr.MAX_TARGETS + 1, targets=(target(),) * (mr.MAX_TARGETS + 1))], None),
        ("null targets", [morph(null_targets=True, nt=1)], None),
        ("removing with a pointer", [morph(nt=0)], None),
        ("reserved", [morph(reserved=1)], None), ("target reserved", [morph(targets=(target(reserved=1),))], None),
        ("more entries than vertices", [morph(targets=(target(count=n4 + 1, index=None, d=np.ones((n4 + 1, 3), F)),))], None),
        ("no indices, an entry fewer", [morph(targets=(target(count=n4 - 1, index=None, d=dense),))], None),
        ("no indices, one entry", [morph(targets=(target(count=1, index=None, d=dense),))], None),
        ("null delta", [morph(targets=(target(d=None),))], None), ("dense and null delta", [morph(targets=(target(count=n4, index=None, d=None),))], None),
        ("an index twice", [morph(targets=(target(index=with_entry(idx, 3, idx[2])),))], None),
        ("indices descending", [morph(targets=(target(index=with_entry(idx, 3, idx[1])),))], None),
        ("index of the vertex count", [morph(targets=(target(index=with_entry(idx, len(idx) - 1, n4)),))], None),
        ("index 2^32 - 1", [morph(targets=(target(index=with_entry(idx, 0, 0xffffffff)),))], None),
        ("delta nan", [morph(targets=(target(d=with_entry(delta, 4, nan)),))], None), ("delta inf", [morph(targets=(target(d=with_entry(delta, 0, inf)),))], None),
        ("delta -inf", [morph(targets=(target(d=with_entry(delta, 3 * len(idx) - 1, -inf)),))], None),
        ("the third target is bad", [morph(targets=(target(), target(count=n4, index=None, d=dense), target(d=with_entry(delta, 1, nan))))], None),
        ("the second mesh is bad", [morph(mesh=3, nv=n3, targets=(target(count=n3, index=None, d=np.ones((n3, 3), F)),)), morph(targets=(target(reserved=7),))], None),
    ])


def pack_morphs(entries):
    """(the array, what it points to)"""
    s, keep = (abi.MeshMorph * max(1, len(entries)))(), []
    for k, e in enumerate(entries):
        s[k].mesh, s[k].num_vertices, s[k].num_targets, s[k]._reserved = e["mesh"], e["nv"], e["nt"], e["reserved"]
        if e["targets"] is not None:
            ts = (abi.MorphTarget * max(1, len(e["targets"])))()
            for t, T in enumerate(e["targets"]):
                ts[t].count, ts[t]._reserved, ts[t].index, ts[t].delta = T["count"], T["reserved"], _ptr(T["index"]), _ptr(T["delta"])
            keep.append(ts)
            s[k].targets = ts
    return s, keep


def morph_pose_cases(base, morphs, weights):
    """(name, entries, num, flags, rule): entries of dict(mesh, nt, weights, nj, reserved, m); rule as in skin_pose_cases."""
    W4, W3 = np.ascontiguousarray(cornell_weights(0.5)[4]), np.ascontiguousarray(weights[3])      # (a good entry would move the block)
    P4, P3 = np.ascontiguousarray(sk.bend_pose(base.meshes[4].vertex, 3, 20.0, (1.0, 2.0, 3.0))), np.ascontiguousarray(tf.IDENTITY[None])
    A5 = float(np.abs(base.meshes[5].vertex).max())
    assert 0 < A5 < 2.0 ** 20                                             # B of mesh 5 is A5 + |w| 2^100 in binary64: at |w| = 2^27 the sum
    over27 = above(2.0 ** 27)                                             # rounds to 2^127 (A5 is below half an ulp); one ulp more is above
    assert A5 + 2.0 ** 127 == 2.0 ** 127 and mr.bound(base.meshes[5].vertex, morphs[5], F([over27])) == 2.0 ** 127 + 2.0 ** 104
    assert 400 < np.abs(base.meshes[4].vertex).max() < 600

    def pose(mesh=4, nt=4, wts=W4, nj=0, reserved=0, m=None):
        return dict(mesh=mesh, nt=nt, weights=wts, nj=nj, reserved=reserved, m=m)

    return names_are_unique([
        ("num below 0", [pose()], -1, 0, False),
        ("mesh above", [pose(mesh=6)], None, 0, False), ("mesh below", [pose(mesh=-1)], None, 0, False),
        ("listed twice", [pose(), pose()], None, 0, False),
        ("a mesh without morphs", [pose(mesh=2)], None, 0, False),
        ("fewer targets than the mesh", [pose(nt=3)], None, 0, False), ("more targets than the mesh", [pose(nt=5)], None, 0, False),
        ("null weights", [pose(wts=None)], None, 0, False), ("null device weights", [pose(wts=None)], None, abi.UPDATE_DEVICE, False),
        ("flag 4", [pose()], None, 4, False), ("flag 8 with rebuild", [pose()], None, 8 | abi.UPDATE_REBUILD, False),
        ("reserved", [pose(reserved=1)], None, 0, False),
        ("matrices on a mesh without a skin", [pose(mesh=5, nt=1, wts=F([0.5]), nj=1, m=P3)], None, 0, False),
        ("fewer joints than the skin", [pose(nj=2, m=P4)], None, 0, False), ("more joints than the skin", [pose(nj=4, m=P4)], None, 0, False),
        ("joints and null matrices", [pose(nj=3)], None, 0, False), ("matrices and no joints", [pose(m=P4)], None, 0, False),
        ("joints and null device matrices", [pose(nj=3)], None, abi.UPDATE_DEVICE, False),
        ("weight nan", [pose(wts=with_entry(W4, 1, nan))], None, 0, True), ("weight inf", [pose(wts=with_entry(W4, 3, inf))], None, 0, True),
        ("weight -inf with rebuild", [pose(wts=with_entry(W4, 0, -inf))], None, abi.UPDATE_REBUILD, True),
        ("matrix nan", [pose(nj=3, m=with_entry(P4, 5, nan))], None, 0, True), ("matrix -inf", [pose(nj=3, m=with_entry(P4, 35, -inf))], None, 0, True),
        ("positions above the bound", [pose(mesh=5, nt=1, wts=F([over27]))], None, 0, True),      # B = A + (2^27 + 2^4) 2^100 > 2^127
        ("positions above the bound, negative weight", [pose(mesh=5, nt=1, wts=F([-over27]))], None, 0, True),
        ("row above the bound", [pose(nj=3, m=with_entry(P4, 2, 1e36))], None, 0, True),      # 1e36 B > 2^127 = 1.7e38 (B is above 400)
        ("translation above the bound", [pose(nj=3, m=with_entry(P4, 19, 1.8e38))], None, 0, True),
        ("S 4, an ulp above 2^125", [pose(mesh=3, nt=1, wts=W3, nj=1, m=row_only(above(2.0 ** 125)))], None, 0, True),
        ("S 4, a blended entry of 2^128", [pose(mesh=3, nt=1, wts=W3, nj=1, m=with_entry(P3, 1, 2.0 ** 126))], None, 0, True),
        ("the second pose is bad", [pose(), pose(mesh=3, nt=1, wts=with_entry(W3, 0, nan))], None, 0, True),
    ])


def pack_morph_poses(entries):
    p = (abi.MorphPose * max(1, len(entries)))()
    for k, e in enumerate(entries):
        p[k].mesh, p[k].num_targets, p[k].weights = e["mesh"], e["nt"], _ptr(e["weights"])
        p[k].num_joints, p[k]._reserved, p[k].matrices = e["nj"], e["reserved"], _ptr(e["m"])
    return p


# ---- fovpt_update_transforms ----------------------------------------------------------------------------------------------------
TRANSFORM_GOOD = tf.rotation_translation(10.0, (368.0, 0.0, 351.0), (5.0, 0.0, 0.0))


def transform_cases(base):
    """(name, entries, num, flags, rule): entries of (mesh, 12 floats)."""
    good = np.asarray(TRANSFORM_GOOD, F).reshape(-1)
    ok = (4, good)
    assert 400 < np.abs(base.meshes[4].vertex).max() < 500
    return names_are_unique([
        ("num below 0", [ok], -1, 0, False),
        ("mesh above", [(6, good)], None, 0, False), ("mesh below", [(-1, good)], None, 0, False),
        ("listed twice", [ok, ok], None, 0, False),
        ("flag 1 is fovpt_update_vertices' alone", [ok], None, abi.UPDATE_DEVICE, False),
        ("flag 1 with rebuild", [ok], None, abi.UPDATE_DEVICE | abi.UPDATE_REBUILD, False),
        ("flag 4", [ok], None, 4, False),
        ("entry nan", [(4, with_entry(good, 5, nan))], None, 0, True), ("entry inf", [(4, with_entry(good, 0, inf))], None, 0, True),
        ("entry -inf with rebuild", [(4, with_entry(good, 11, -inf))], None, abi.UPDATE_REBUILD, True),
        ("row above the bound", [(4, with_entry(good, 2, 1e36))], None, 0, True),       # 1e36 A > 2^127 = 1.7e38 (the block's A is between 400 and 500)
        ("translation above the bound", [(4, with_entry(good, 7, 1.8e38))], None, 0, True),
        ("the second transform is bad", [ok, (3, with_entry(good, 9, nan))], None, 0, True),      # nothing of the first is applied
    ])


def pack_transforms(entries):
    tfs = (abi.MeshTransform * max(1, len(entries)))()
    for k, (mesh, m) in enumerate(entries):
        tfs[k].mesh = mesh
        tfs[k].m[:] = [float(x) for x in np.asarray(m, F).reshape(-1)]
    return tfs


# ---- fovpt_set_rig ------------------------------------------------------------------------------------------------------------------
def rig_skins(model):
    return {TALL: sk.bend(model.meshes[TALL].vertex, 3)}


def cornell_rig(model):
    """The tall block on a chain of three joints up its height, the short block rigid on node 4, which hangs from a pivot (node
    3) at the block's centre.  Clip 0 has translation, rotation and scale channels of 2 to 4 keys, STEP and LINEAR, with rotation
    keys 20 degrees apart (the sine branch), 2 degrees apart (the linear one) and on opposite hemispheres (the flip); clip 1
    moves the short block alone."""
    rig = rg.empty_rig(5)
    rig["parent"] = np.array([-1, 0, 1, -1, 3], np.int32)
    rig["translation"] = F([[368, 0, 351], [0, 110, 0], [0, 110, 0], [186, 82, 168], [-186, -82, -168]])
    rig["rotation"][0] = rg.quat((0, 1, 0), 15.0)
    z = (0.1, 0.0, 1.0)
    rig["clips"] = [[
        rg.channel(0, rg.ROTATION, [0.0, 1.0, 2.0], [rg.quat(z, 0.0), rg.quat(z, 20.0), rg.quat(z, 22.0)]),
        rg.channel(1, rg.TRANSLATION, [0.5, 1.5], [[0, 110, 0], [12, 100, -6]]),
        rg.channel(1, rg.ROTATION, [0.0, 0.5, 1.0, 1.5], [rg.quat((1, 0, 0), 0.0), -rg.quat((1, 0, 0), 14.0), rg.quat((1, 0, 0.3), 15.0, 1.3), rg.quat((1, 0, 0.3), 16.5, 0.8)]),
        rg.channel(2, rg.SCALE, [0.25, 1.75], [[1, 1, 1], [1.2, 0.9, 1.1]]),
        rg.channel(2, rg.ROTATION, [0.5, 1.0, 2.0], [rg.quat((0, 0, 1), -10.0), rg.quat((0, 0, 1), 10.0), rg.quat((0, 1, 0), 30.0)], rg.STEP),
        rg.channel(3, rg.TRANSLATION, [0.0, 1.0, 2.0], [[186, 82, 168], [150, 95, 190], [160, 120, 150]], rg.STEP),
        rg.channel(3, rg.ROTATION, [0.0, 2.0], [rg.quat((0, 1, 0), 0.0), rg.quat((0, 1, 0), 50.0)]),
        rg.channel(3, rg.SCALE, [0.0, 1.0, 1.25, 2.0], [[1, 1, 1], [1.1, 0.8, 1], [1.1, 0.8, 1.2], [0.9, 1, 1]]),
    ], [rg.channel(3, rg.TRANSLATION, [0.0, 1.0], [[186, 82, 168], [200, 82, 140]])]]
    rig["bindings"] = [dict(mesh=TALL, joint_nodes=np.array([0, 1, 2], np.uint16), inverse_bind=rg.inverse_bind_of(rig, [0, 1, 2])), dict(mesh=SHORT, node=4)]
    return rig


def rig_morph_fixture(model):
    """The tall block skinned and morphed (4 targets), the short block morphed alone (3 targets), the left wall rigid."""
    rng = np.random.default_rng(7)
    skins = rig_skins(model)
    morphs = {TALL: mr.random_targets(rng, model.meshes[TALL].vertex.shape[0], 4, dense=1, scale=30.0),
              SHORT: mr.random_targets(rng, model.meshes[SHORT].vertex.shape[0], 3, dense=3, scale=20.0)}
    rig = cornell_rig(model)
    rig["bindings"][1] = dict(mesh=SHORT)
    rig["bindings"].append(dict(mesh=2, node=3))
    rig["clips"][0] += [rg.channel(TALL, rg.WEIGHTS, [0.0, 1.0, 2.0], [[0, 0, 0, 0], [1, -0.5, 0, 2], [0, 0.25, 0, 1]]),
                        rg.channel(SHORT, rg.WEIGHTS, [0.5, 1.5], [[0, 1, 0], [1, 0, -1]], rg.STEP)]
    rig["clips"][1] = [rg.channel(0, rg.ROTATION, [0.0, 1.0], [rg.quat((0, 0, 1), 0.0), rg.quat((0, 0, 1), 25.0)])]       # no WEIGHTS channel
    return skins, morphs, rig


def rig_scene(model):
    """(skins, morphs, rig) the rejection test sets first: rig_morph_fixture, and morphs on mesh 5 and a skin on mesh 1 that the rig
    does not bind."""
    skins, morphs, rig = rig_morph_fixture(model)
    morphs[5] = mr.random_targets(np.random.default_rng(2), model.meshes[5].vertex.shape[0], 1)
    skins[1] = sk.bend(model.meshes[1].vertex, 2)
    return skins, morphs, rig


def describe_rig(rig):
    """The plain description of a rig of rig_ref's form: the counts as stated fields beside the arrays they count, None for a null
    pointer, the reserved fields."""
    n = len(rig["parent"])
    nodes = [dict(parent=int(rig["parent"][i]), translation=np.array(rig["translation"][i], F), rotation=np.array(rig["rotation"][i], F),
                  scale=np.array(rig["scale"][i], F)) for i in range(n)]
    bindings = []
    for b in rig.get("bindings", ()):
        jn = b.get("joint_nodes")
        bindings.append(dict(mesh=int(b["mesh"]), node=int(b.get("node", -1)), num_joints=0 if jn is None else len(jn), reserved=0,
                             joint_nodes=None if jn is None else np.array(jn, np.uint16), inverse_bind=None if jn is None else sk.palette(b["inverse_bind"]).copy()))
    clips = [dict(num_channels=len(clip), reserved=0,
                  channels=[dict(target=int(c["target"]), path=int(c["path"]), interpolation=int(c["interpolation"]), num_keys=len(c["times"]),
                                 times=np.array(c["times"], F), values=np.array(c["values"], F).reshape(len(c["times"]), -1)) for c in clip]) for clip in rig.get("clips", ())]
    return dict(reserved0=0, reserved1=0, reserved2=0, num_nodes=n, nodes=nodes, num_bindings=len(bindings), bindings=bindings, num_clips=len(clips), clips=clips)


def pack_rig(d):
    """(abi.RigDesc, what it points to) of a description.  An array is as long as the description holds it, whatever the count
    beside it says."""
    keep = []

    def held(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a.ctypes.data

    desc = abi.RigDesc()
    desc.num_nodes, desc.num_bindings, desc.num_clips = d["num_nodes"], d["num_bindings"], d["num_clips"]
    desc._reserved0, desc._reserved1, desc._reserved2 = d["reserved0"], d["reserved1"], d["reserved2"]
    if d["nodes"] is not None:
        nodes = (abi.RigNode * max(1, len(d["nodes"])))()
        for i, N in enumerate(d["nodes"]):
            nodes[i].parent = N["parent"]
            nodes[i].translation[:], nodes[i].rotation[:], nodes[i].scale[:] = [float(x) for x in N["translation"]], [float(x) for x in N["rotation"]], [float(x) for x in N["scale"]]
        keep.append(nodes)
        desc.nodes = nodes
    if d["bindings"] is not None:
        bs = (abi.RigBinding * max(1, len(d["bindings"])))()
        for k, B in enumerate(d["bindings"]):
            bs[k].mesh, bs[k].node, bs[k].num_joints, bs[k]._reserved = B["mesh"], B["node"], B["num_joints"], B["reserved"]
            bs[k].joint_nodes, bs[k].inverse_bind = held(B["joint_nodes"]), held(B["inverse_bind"])
        keep.append(bs)
        desc.bindings = bs
    if d["clips"] is not None:
        cs = (abi.RigClip * max(1, len(d["clips"])))()
        for k, K in enumerate(d["clips"]):
            cs[k].num_channels, cs[k]._reserved = K["num_channels"], K["reserved"]
            if K["channels"] is not None:
                ch = (abi.RigChannel * max(1, len(K["channels"])))()
                for h, H in enumerate(K["channels"]):
                    ch[h].target, ch[h].path, ch[h].interpolation, ch[h].num_keys = H["target"], H["path"], H["interpolation"], H["num_keys"]
                    ch[h].times, ch[h].values = held(H["times"]), held(H["values"])
                keep.append(ch)
                cs[k].channels = ch
        keep.append(cs)
        desc.clips = cs
    return desc, keep


def _walk(d, path):
    keys = [int(k[1:-1]) if k[0] == "[" else k for k in re.findall(r"\[\d+\]|\w+", path)]
    for k in keys[:-1]:
        d = d[k]
    return d, keys[-1]


def put(path, value):
    """The change desc.<path> = value, path like 'bindings[1].node' or 'clips[0].channels[2].times'; value may be a function of the
    description."""
    def change(d):
        at, key = _walk(d, path)
        at[key] = value(d) if callable(value) else value
    return change


def entry(path, index, value):
    """The change of one entry, counted over the flattened array, of the array at <path>."""
    def change(d):
        at, key = _walk(d, path)
        at[key] = with_entry(at[key], index, value)
    return change


def changed(desc, changes):
    d = copy.deepcopy(desc)
    for change in changes:
        change(d)
    return d


def rig_cases(rig):
    """(name, changes) over describe_rig(rig) of rig_scene()'s rig."""
    B, CH = "bindings[%d].%s", "clips[0].channels[%d].%s"
    assert len(rig["clips"][0]) == 10 and rig["clips"][0][8]["path"] == rig["clips"][0][9]["path"] == rg.WEIGHTS
    # clip 0's channels: 0 R(node 0) 1 T(1) 2 R(1) 3 S(2) 4 R(2) 5 T(3) 6 R(3) 7 S(3) 8 W(TALL) 9 W(SHORT)
    return names_are_unique([(name, c if isinstance(c, list) else [c]) for name, c in [
        # the description as a whole
        ("reserved0", put("reserved0", 1)), ("reserved1", put("reserved1", 1)), ("reserved2", put("reserved2", 7)),
        ("no nodes", put("num_nodes", 0)), ("too many nodes", put("num_nodes", rg.MAX_NODES + 1)), ("too many clips", put("num_clips", rg.MAX_CLIPS + 1)),
        ("null nodes", put("nodes", None)), ("null bindings", put("bindings", None)), ("null clips", put("clips", None)),
        ("clip reserved", put("clips[1].reserved", 1)), ("null channels", put("clips[0].channels", None)),
        # nodes
        ("parent is itself", put("nodes[2].parent", 2)), ("parent above", put("nodes[1].parent", 3)), ("parent below -1", put("nodes[0].parent", -2)),
        ("rest translation nan", put("nodes[1].translation[2]", nan)), ("rest rotation inf", put("nodes[4].rotation[0]", inf)),
        ("rest scale -inf", put("nodes[3].scale[1]", -inf)),
        ("rest rotation too short", put("nodes[2].rotation[3]", below(0.5))), ("rest rotation too long", put("nodes[2].rotation[3]", above(2.0))),
        # bindings
        ("mesh above", put(B % (0, "mesh"), 6)), ("mesh below", put(B % (0, "mesh"), -1)), ("bound twice", put(B % (2, "mesh"), TALL)),
        ("binding reserved", put(B % (1, "reserved"), 1)),
        ("node and joints", put(B % (0, "node"), 1)), ("node above", put(B % (2, "node"), 5)), ("node below -1", put(B % (2, "node"), -2)),
        ("joint node above", put(B % (0, "joint_nodes"), np.array([0, 5, 2], np.uint16))),
        ("fewer joints than the skin", put(B % (0, "num_joints"), 2)), ("more joints than the skin", put(B % (0, "num_joints"), 4)),
        ("joints on a mesh without a skin", [put(B % (2, "node"), -1), put(B % (2, "num_joints"), 3),
                                             put(B % (2, "joint_nodes"), lambda d: d["bindings"][0]["joint_nodes"].copy()),
                                             put(B % (2, "inverse_bind"), lambda d: d["bindings"][0]["inverse_bind"].copy())]),
        ("rigid and morphs", put(B % (1, "node"), 2)),
        ("neither node, joints nor morphs", put(B % (2, "node"), -1)),
        ("null joint_nodes", put(B % (0, "joint_nodes"), None)), ("null inverse_bind", put(B % (0, "inverse_bind"), None)),
        ("inverse bind nan", entry(B % (0, "inverse_bind"), 17, nan)), ("inverse bind inf", entry(B % (0, "inverse_bind"), 35, -inf)),
        # clips and channels
        ("path above", put(CH % (1, "path"), 4)), ("path below", put(CH % (1, "path"), -1)),
        ("interpolation above", put(CH % (1, "interpolation"), 2)), ("interpolation below", put(CH % (1, "interpolation"), -1)),
        ("node target above", put(CH % (1, "target"), 5)), ("node target below", put(CH % (1, "target"), -1)),
        ("mesh target above", put(CH % (8, "target"), 6)), ("mesh target below", put(CH % (8, "target"), -1)),
        ("weights of a mesh that is not bound", put(CH % (9, "target"), 5)), ("weights of a bound mesh without morphs", put(CH % (9, "target"), 2)),
        ("weights of a mesh with neither", put(CH % (9, "target"), 0)),
        ("the same node and path twice", put(CH % (3, "target"), 3)), ("the same weights twice", [put(CH % (1, "path"), rg.WEIGHTS), put(CH % (1, "target"), SHORT)]),
        ("no keys", put(CH % (1, "num_keys"), 0)), ("too many keys", put(CH % (1, "num_keys"), rg.MAX_KEYS + 1)),
        ("null times", put(CH % (1, "times"), None)), ("null values", put(CH % (1, "values"), None)),
        ("time nan", put(CH % (0, "times"), F([0, nan, 2]))), ("time inf", put(CH % (0, "times"), F([0, 1, inf]))),
        ("time -inf", put(CH % (0, "times"), F([-inf, 1, 2]))),
        ("times equal", put(CH % (0, "times"), F([0, 1, 1]))), ("times descending", put(CH % (0, "times"), F([0, 2, 1]))),
        ("value nan", entry(CH % (1, "values"), 4, nan)), ("value inf", entry(CH % (3, "values"), 0, inf)), ("weight nan", entry(CH % (8, "values"), 11, nan)),
        ("rotation key too short", put(CH % (0, "values"), np.array([[0, 0, 0, 1], [0, below(0.5), 0, 0], [0, 0, 0, 1]], F))),
        ("rotation key too long", put(CH % (0, "values"), np.array([[0, 0, 0, 1], [0, 0, 0, 1], [above(1.0), 1, 1, 1]], F))),
    ]])


# What rig_ref.accepted deliberately leaves aside: the null pointers, the reserved fields and the counts of the C structs, which a rig
# of its form cannot state
RIG_CASES_BEYOND_THE_RESTATEMENT = (
    "reserved0", "reserved1", "reserved2", "clip reserved", "binding reserved", "no nodes", "too many nodes", "too many clips", "null nodes",
    "null bindings", "null clips", "null channels", "null joint_nodes", "null inverse_bind", "null times", "null values",
    "fewer joints than the skin", "more joints than the skin", "no keys", "too many keys")


def rig_of(d):
    """A description in rig_ref's form again (for rig_ref.accepted), where it can be stated in that form."""
    rig = dict(parent=np.array([N["parent"] for N in d["nodes"]], np.int32), translation=np.stack([N["translation"] for N in d["nodes"]]),
               rotation=np.stack([N["rotation"] for N in d["nodes"]]), scale=np.stack([N["scale"] for N in d["nodes"]]), bindings=[], clips=[])
    for B in d["bindings"]:
        b = dict(mesh=B["mesh"], node=B["node"])
        if B["num_joints"]:
            b.update(joint_nodes=B["joint_nodes"], inverse_bind=B["inverse_bind"].reshape(-1, 3, 4))
        rig["bindings"].append(b)
    for K in d["clips"]:
        rig["clips"].append([dict(target=H["target"], path=H["path"], interpolation=H["interpolation"], times=H["times"], values=H["values"]) for H in K["channels"]])
    return rig
