"""CPU tests of tests/rig_ref.py, the restatement fovpt_update_animated is checked against on the GPU: the arithmetic against a
scalar loop that rounds after every operation, the sampling rules, identity and closed-form rigs, an independent binary64
statement, the validation rules on either side, and the ABI mirrors of the rig structs.

Measured on this file's binary64 comparison (seeds 0 .. 11, depth up to 16, rotations and unit scales): the largest absolute error
of a world or palette entry is 4.93e-7 of the rig's largest |entry|; the test asserts four times that."""
import ctypes

import numpy as np
import pytest

import header_layout
import rig_ref as rg
from fovpathtracing_optixcodelatest_amd import abi

F = np.float32
MEASURED_F64_ERROR = 4.93e-7


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the scalar loop -------------------------------------------------------------------------------------------------------------
def _sin(oracle, x):
    return oracle.math_op(rg.OP_SIN, np.array([x], F))[0]


def _scalar_sample(oracle, ch, T):
    t, v = [F(x) for x in ch["times"]], np.asarray(ch["values"], F).reshape(len(ch["times"]), -1)
    T = F(T)
    if T <= t[0]:
        return [F(x) for x in v[0]]
    if T >= t[-1]:
        return [F(x) for x in v[-1]]
    k = max(i for i in range(len(t)) if t[i] <= T)
    if ch["interpolation"] == rg.STEP:
        return [F(x) for x in v[k]]
    u = F(F(T - t[k]) / F(t[k + 1] - t[k]))
    a, b = [F(x) for x in v[k]], [F(x) for x in v[k + 1]]
    if ch["path"] != rg.ROTATION:
        return [F(a[e] + F(u * F(b[e] - a[e]))) for e in range(len(a))]
    d = F(F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2])) + F(a[3] * b[3]))
    if d < 0:
        b, d = [F(-x) for x in b], F(-d)
    if d > F(0.9995):
        q = [F(a[e] + F(u * F(b[e] - a[e]))) for e in range(4)]
    else:
        th = oracle.math_op(rg.OP_ACOS, np.array([d], F))[0]
        s = _sin(oracle, th)
        wa = F(_sin(oracle, F(F(F(1.0) - u) * th)) / s)
        wb = F(_sin(oracle, F(u * th)) / s)
        q = [F(F(wa * a[e]) + F(wb * b[e])) for e in range(4)]
    n = F(np.sqrt(F(F(F(F(q[0] * q[0]) + F(q[1] * q[1])) + F(q[2] * q[2])) + F(q[3] * q[3]))))
    return [F(x / n) for x in q]


def _scalar_compose(P, L):
    out = [[None] * 4 for _ in range(3)]
    for r in range(3):
        for c in range(3):
            out[r][c] = F(F(F(P[r][0] * L[0][c]) + F(P[r][1] * L[1][c])) + F(P[r][2] * L[2][c]))
        out[r][3] = F(F(F(F(P[r][0] * L[0][3]) + F(P[r][1] * L[1][3])) + F(P[r][2] * L[2][3])) + P[r][3])
    return out


def _scalar_pose(oracle, rig, clip, T):
    """(world, palettes, rigid) one operation at a time, every result rounded to binary32."""
    n = len(rig["parent"])
    one, two = F(1.0), F(2.0)
    trs = {(i, p): [F(x) for x in rig[name][i]] for i in range(n) for p, name in enumerate(("translation", "rotation", "scale"))}
    for ch in rig["clips"][clip]:
        if ch["path"] != rg.WEIGHTS:
            trs[(ch["target"], ch["path"])] = _scalar_sample(oracle, ch, T)
    world = []
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for i in range(n):
            t, (x, y, z, w), s = trs[(i, 0)], trs[(i, 1)], trs[(i, 2)]
            r = [[F(one - F(two * F(F(y * y) + F(z * z)))), F(two * F(F(x * y) - F(z * w))), F(two * F(F(x * z) + F(y * w)))],
                 [F(two * F(F(x * y) + F(z * w))), F(one - F(two * F(F(x * x) + F(z * z)))), F(two * F(F(y * z) - F(x * w)))],
                 [F(two * F(F(x * z) - F(y * w))), F(two * F(F(y * z) + F(x * w))), F(one - F(two * F(F(x * x) + F(y * y))))]]
            L = [[F(r[a][c] * s[c]) for c in range(3)] + [t[a]] for a in range(3)]
            p = int(rig["parent"][i])
            world.append(L if p < 0 else _scalar_compose(world[p], L))
        palettes, rigid = [], []
        for b in rig["bindings"]:
            if b.get("joint_nodes") is not None:
                ib = np.asarray(b["inverse_bind"], F).reshape(-1, 3, 4)
                palettes.append(np.array([_scalar_compose(world[int(j)], [[F(e) for e in row] for row in ib[k]]) for k, j in enumerate(b["joint_nodes"])], F))
            elif b.get("node", -1) >= 0:
                rigid.append(np.array(world[b["node"]], F))
    return np.array(world, F), palettes, rigid


def _bind_some(rng, rig, num_skinned=2, joints=5):
    n = len(rig["parent"])
    rig["bindings"] = []
    for m in range(num_skinned):
        nodes = rng.integers(0, n, joints).astype(np.uint16)
        rig["bindings"].append(dict(mesh=m, joint_nodes=nodes, inverse_bind=rg.inverse_bind_of(rig, nodes)))
    rig["bindings"].append(dict(mesh=num_skinned, node=int(rng.integers(0, n))))
    return rig


def _edge_rig():
    """+-0 and 1e+-30 translations, scales far from 1, a three-deep chain and two roots."""
    rig = rg.empty_rig(5)
    rig["parent"] = np.array([-1, 0, 1, -1, 3], np.int32)
    rig["translation"] = F([[0.0, -0.0, 1e-30], [-0.0, 1e30, -1e-30], [1e-30, -1e30, 0.0], [-0.0, -0.0, -0.0], [1e30, 1e-30, -0.0]])
    rig["scale"] = F([[1e-3, 2.5, -1.0], [3.0, 1e-3, 0.5], [1.0, 1.0, 1.0], [-0.0, 0.0, 1e3], [7.0, -0.25, 1e-3]])
    rig["rotation"] = np.stack([rg.quat((1, 2, 3), 40.0), rg.quat((0, 1, 0), -90.0), F([0, 0, 0, 1]), rg.quat((1, 0, 0), 180.0, 1.9), rg.quat((1, 1, 0), 10.0, 0.55)])
    rig["clips"] = [[rg.channel(1, rg.TRANSLATION, [0.0, 1.0], [[-0.0, 1e30, -1e-30], [1e-30, -1e30, 0.0]]),
                     rg.channel(4, rg.SCALE, [0.0, 2.0], [[1e-3, 1e3, -0.0], [-1e-3, 0.0, 2.0]])]]
    rig["bindings"] = [dict(mesh=0, joint_nodes=np.array([2, 4, 0], np.uint16), inverse_bind=np.tile(np.eye(3, 4, dtype=F), (3, 1, 1))), dict(mesh=1, node=2)]
    return rig


def _pose_cases():
    out = {}
    for seed in range(4):
        rng = np.random.default_rng(20 + seed)
        out["random%d" % seed] = _bind_some(rng, rg.random_rig(rng, 12 + 9 * seed, max_depth=(None, 4, 8, 16)[seed]))
    out["edge"] = _edge_rig()
    return out


POSE_CASES = _pose_cases()


@pytest.mark.parametrize("name", sorted(POSE_CASES))
def test_pose_is_the_scalar_expression(oracle, name):
    rig = POSE_CASES[name]
    assert rg.accepted(rig, 3, skins={0: len(rig["bindings"][0]["joint_nodes"]), 1: 5})
    for T in (-1.0, 0.0, 0.3, 0.77, 1.0, 1.9, 5.0):
        got = rg.pose(oracle, rig, 0, T)
        world, palettes, rigid = _scalar_pose(oracle, rig, 0, T)
        assert np.array_equal(_bits(got["world"]), _bits(world)), T
        assert len(got["palettes"]) == len(palettes) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got["palettes"], palettes))
        assert len(got["rigid"]) == len(rigid) == 1 and np.array_equal(_bits(got["rigid"][0]), _bits(rigid[0]))
    if name == "edge":
        assert np.isfinite(got["world"]).all() and (np.abs(got["world"]) > 1e29).any() and (got["world"] == 0).any()


# ---- sampling ------------------------------------------------------------------------------------------------------------------
def test_sampling_before_at_between_and_after_every_key(oracle):
    times = F([0.5, 1.0, 1.75, 4.0])
    vals = F([[1, -0.0, 3], [2, 5, -0.0], [-4, 5, 0.5], [8, -0.0, 1]])
    lin, step = rg.channel(0, rg.TRANSLATION, times, vals), rg.channel(0, rg.TRANSLATION, times, vals, rg.STEP)
    for ch in (lin, step):                                               # the ends: the key as given, -0 included
        for T in (-3.0, 0.5, np.nextafter(F(0.5), F(0))):
            assert np.array_equal(_bits(rg.sample(oracle, ch, T)), _bits(vals[0]))
        for T in (4.0, np.nextafter(F(4.0), F(9)), 1e30):
            assert np.array_equal(_bits(rg.sample(oracle, ch, T)), _bits(vals[3]))
    for k in (1, 2):
        # STEP: the key from its time up to just before the next one, bit for bit
        for T in (times[k], np.nextafter(times[k + 1], F(0))):
            assert np.array_equal(_bits(rg.sample(oracle, step, T)), _bits(vals[k]))
        assert np.array_equal(_bits(rg.sample(oracle, step, np.nextafter(times[k], F(0)))), _bits(vals[k - 1]))
        # LINEAR at an interior key: u = 0, v_k + 0 * (v_{k+1} - v_k): the key's value, but a component of -0 becomes +0
        at = rg.sample(oracle, lin, times[k])
        assert np.array_equal(at, vals[k]) and np.array_equal(_bits(at), _bits(vals[k] + F(0.0)))
    assert _bits(rg.sample(oracle, lin, times[1]))[2] == 0 and _bits(vals[1])[2] == 0x80000000
    # between keys: u and the lerp, one operation at a time
    T = F(1.3)
    u = F(F(T - times[1]) / F(times[2] - times[1]))
    want = F([F(vals[1][e] + F(u * F(vals[2][e] - vals[1][e]))) for e in range(3)])
    assert np.array_equal(_bits(rg.sample(oracle, lin, T)), _bits(want))
    assert rg.locate(times, T) == (1, u) and rg.locate(times, 0.4) == (0, None) and rg.locate(times, 4.0) == (3, None)
    assert rg.locate(times, np.nextafter(F(4.0), F(0)))[0] == 2
    # one key: that key at every time, under either interpolation
    one = rg.channel(0, rg.ROTATION, [2.0], [[0, 0, 0.6, 0.9]])
    for T in (0.0, 2.0, 7.0):
        assert np.array_equal(_bits(rg.sample(oracle, one, T)), _bits(F([0, 0, 0.6, 0.9])))
    # weights: as wide as the mesh has targets
    wch = rg.channel(0, rg.WEIGHTS, [0.0, 2.0], [[0, 1, -0.5, 0, 2], [1, 1, 0.5, 0, -2]])
    assert np.array_equal(rg.sample(oracle, wch, 1.0), F([0.5, 1, 0, 0, 0]))


def test_slerp_flip_and_the_two_branches(oracle):
    a = rg.quat((0, 0, 1), 0.0)
    near, far = rg.quat((0, 0, 1), 3.0), rg.quat((0, 0, 1), 4.0)          # cos(1.5 deg) = 0.99966, cos(2 deg) = 0.99939
    dot = lambda p, q: F(F(F(F(p[0] * q[0]) + F(p[1] * q[1])) + F(p[2] * q[2])) + F(p[3] * q[3]))
    assert dot(a, near) > F(0.9995) > dot(a, far) > 0
    u = F(0.25)
    got = rg.slerp(oracle, a, near, u)                                    # the linear branch, then the division by the norm
    q = a + u * (near - a)
    n = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    assert np.array_equal(_bits(got), _bits(q / n))
    got = rg.slerp(oracle, a, far, u)                                     # the sine branch
    th = oracle.math_op(rg.OP_ACOS, np.array([dot(a, far)], F))[0]
    s = _sin(oracle, th)
    q = (_sin(oracle, (F(1.0) - u) * th) / s) * a + (_sin(oracle, u * th) / s) * far
    n = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    assert np.array_equal(_bits(got), _bits(q / n))
    assert np.allclose(got.astype(np.float64), rg.quat((0, 0, 1), 1.0).astype(np.float64), atol=2e-7)
    # d < 0: the short way round, through -b
    for b in (near, far, rg.quat((1, 0, 0), 120.0)):
        assert dot(a, -b) < 0
        assert np.array_equal(_bits(rg.slerp(oracle, a, -b, u)), _bits(rg.slerp(oracle, a, b, u)))
    # the sine branch at its widest: d = 0, theta = pi / 2
    half = rg.slerp(oracle, a, rg.quat((0, 0, 1), 180.0), F(0.5))
    assert np.allclose(half.astype(np.float64), rg.quat((0, 0, 1), 90.0).astype(np.float64), atol=2e-7)
    # through a channel: the ends are not normalised, everything between is
    ch = rg.channel(0, rg.ROTATION, [0.0, 1.0], [a * F(1.5), far * F(0.75)])
    assert np.array_equal(_bits(rg.sample(oracle, ch, 0.0)), _bits(a * F(1.5))) and np.array_equal(_bits(rg.sample(oracle, ch, 1.0)), _bits(far * F(0.75)))
    mid = rg.sample(oracle, ch, 0.5).astype(np.float64)
    assert abs((mid * mid).sum() - 1.0) < 1e-6
    step = dict(ch, interpolation=rg.STEP)
    assert np.array_equal(_bits(rg.sample(oracle, step, 0.5)), _bits(a * F(1.5)))


# ---- whole rigs --------------------------------------------------------------------------------------------------------------------
def test_identity_rig_leaves_the_inverse_bind(oracle):
    rng = np.random.default_rng(3)
    rig = rg.empty_rig(6)
    rig["parent"] = np.array([-1, 0, 1, 1, -1, 4], np.int32)
    ib = rng.uniform(-5, 5, (4, 3, 4)).astype(F)
    ib[0, 1, 2], ib[2, 0, 3] = -0.0, -0.0
    rig["bindings"] = [dict(mesh=0, joint_nodes=np.array([3, 5, 0, 2], np.uint16), inverse_bind=ib)]
    P = rg.pose(oracle, rig, 0, 0.5)
    assert np.array_equal(P["world"], np.tile(np.eye(3, 4, dtype=F), (6, 1, 1)))
    assert np.array_equal(P["palettes"][0], ib)                           # equal, up to the sign of zero:
    assert not np.array_equal(_bits(P["palettes"][0]), _bits(ib)) and np.array_equal(_bits(P["palettes"][0]), _bits(ib + F(0.0)))


def test_one_root_turning_about_an_axis(oracle):
    rig = rg.empty_rig(1)
    rig["translation"][0] = (3.0, -1.0, 2.0)
    rig["clips"] = [[rg.channel(0, rg.ROTATION, [0.0, 2.0], [rg.quat((0, 1, 0), 0.0), rg.quat((0, 1, 0), 120.0)])]]
    rig["bindings"] = [dict(mesh=0, node=0)]
    for T, deg in ((0.0, 0.0), (0.5, 30.0), (1.0, 60.0), (1.7, 102.0), (2.0, 120.0), (3.0, 120.0)):
        a = np.deg2rad(deg)
        want = np.array([[np.cos(a), 0, np.sin(a), 3.0], [0, 1, 0, -1.0], [-np.sin(a), 0, np.cos(a), 2.0]])
        P = rg.pose(oracle, rig, 0, T)
        assert np.abs(P["world"][0].astype(np.float64) - want).max() < 8 * 2.0 ** -24, T      # a few roundings of entries within [-1, 1]
        assert np.array_equal(_bits(P["rigid"][0]), _bits(P["world"][0]))


def _pose64(rig, clip, T):
    """Steps 1 to 4 in plain binary64 with libm's sine and arc cosine: written from the definition, sharing no code with rig_ref."""
    n = len(rig["parent"])
    T = float(F(T))
    trs = [np.array(rig[k], np.float64).reshape(n, -1) for k in ("translation", "rotation", "scale")]
    for ch in rig["clips"][clip]:
        t, v = np.asarray(ch["times"], np.float64), np.asarray(ch["values"], np.float64).reshape(len(ch["times"]), -1)
        if T <= t[0]:
            val = v[0]
        elif T >= t[-1]:
            val = v[-1]
        else:
            k = int(np.nonzero(t <= T)[0][-1])
            u = (T - t[k]) / (t[k + 1] - t[k])
            if ch["interpolation"] == rg.STEP:
                val = v[k]
            elif ch["path"] != rg.ROTATION:
                val = v[k] + u * (v[k + 1] - v[k])
            else:
                a, b = v[k], v[k + 1]
                d = float(a @ b)
                if d < 0:
                    b, d = -b, -d
                if d > float(F(0.9995)):
                    q = a + u * (b - a)
                else:
                    th = np.arccos(d)
                    q = (np.sin((1 - u) * th) * a + np.sin(u * th) * b) / np.sin(th)
                val = q / np.sqrt(q @ q)
        trs[ch["path"]][ch["target"]] = val
    W = np.empty((n, 4, 4))
    for i in range(n):
        x, y, z, w = trs[1][i]
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        L = np.eye(4)
        L[:3, :3], L[:3, 3] = R * trs[2][i][None, :], trs[0][i]
        p = int(rig["parent"][i])
        W[i] = L if p < 0 else W[p] @ L
    pal = []
    for b in rig["bindings"]:
        if b.get("joint_nodes") is not None:
            ib = np.concatenate([np.asarray(b["inverse_bind"], np.float64).reshape(-1, 3, 4), np.tile([[[0, 0, 0, 1.0]]], (len(b["joint_nodes"]), 1, 1))], axis=1)
            pal.append(np.stack([(W[int(j)] @ ib[k])[:3] for k, j in enumerate(b["joint_nodes"])]))
    return W[:, :3], pal


def test_against_an_independent_binary64_statement(oracle):
    """Rotations and unit scales, depth up to 16.  The bound is four times the error measured on these very rigs (module
    docstring): the margin covers other seeds, not a wider class of rigs."""
    worst, deepest = 0.0, 0
    for seed in range(12):
        rng = np.random.default_rng(100 + seed)
        rig = _bind_some(rng, rg.random_rig(rng, 40, max_depth=16, scales=False, chains=0.7))
        deepest = max(deepest, max(_depths(rig)))
        for T in rng.uniform(0.0, 3.0, 4):
            got = rg.pose(oracle, rig, 0, T)
            W, pal = _pose64(rig, 0, T)
            big = max(np.abs(W).max(), max(np.abs(p).max() for p in pal))
            err = max(np.abs(got["world"].astype(np.float64) - W).max(), max(np.abs(g.astype(np.float64) - p).max() for g, p in zip(got["palettes"], pal)))
            worst = max(worst, err / big)
    assert deepest == 16
    print("largest error relative to the largest |entry|: %.3g" % worst)
    assert worst <= 4 * MEASURED_F64_ERROR
    assert worst >= MEASURED_F64_ERROR / 8                                # (the figure in the docstring is still the measured one)


def _depths(rig):
    d = []
    for i, p in enumerate(rig["parent"]):
        d.append(1 if p < 0 else d[int(p)] + 1)
    return d


# ---- validation --------------------------------------------------------------------------------------------------------------------
def _valid():
    """A rig that uses every kind of binding and channel: meshes 0 (skinned, 3 joints), 1 (rigid), 2 (morphs only, 2 targets), 3
    (skinned with 2 joints and 4 targets); mesh 4 is not bound, mesh 5 has morphs and is not bound."""
    rig = rg.empty_rig(4)
    rig["parent"] = np.array([-1, 0, 1, 0], np.int32)
    eye = np.eye(3, 4, dtype=F)
    rig["bindings"] = [dict(mesh=0, joint_nodes=np.array([0, 1, 2], np.uint16), inverse_bind=np.tile(eye, (3, 1, 1))), dict(mesh=1, node=3),
                       dict(mesh=2), dict(mesh=3, joint_nodes=np.array([3, 3], np.uint16), inverse_bind=np.tile(eye, (2, 1, 1)))]
    rig["clips"] = [[rg.channel(1, rg.TRANSLATION, [0, 1], [[0, 0, 0], [1, 2, 3]]), rg.channel(1, rg.ROTATION, [0, 1, 2], [[0, 0, 0, 1], [0, 0, 1, 0], [0, 0.6, 0, 0.8]]),
                     rg.channel(3, rg.SCALE, [0.5], [[1, 2, 1]], rg.STEP), rg.channel(2, rg.WEIGHTS, [0, 1], [[0, 0], [1, 0.5]]),
                     rg.channel(3, rg.WEIGHTS, [0], [[0, 0, 1, 0]])], []]
    return rig


SCENE = dict(num_meshes=6, skins={0: 3, 3: 2}, morphs={2: 2, 3: 4, 5: 1})


def _ok(rig, **scene):
    return rg.accepted(rig, **dict(SCENE, **scene))


def _with(path, value, fn=None):
    """_valid() with rig[path[0]][path[1]]... set to value (or to fn of what is there)."""
    rig = _valid()
    at = rig
    for k in path[:-1]:
        at = at[k]
    at[path[-1]] = fn(at[path[-1]]) if fn else value
    return rig


def test_accepted_on_either_side_of_every_rule():
    assert _ok(_valid())
    below = lambda x: np.nextafter(F(x), F(0))
    above = lambda x: np.nextafter(F(x), F(np.inf))
    # nodes
    assert _ok(rg.empty_rig(1), num_meshes=1) and _ok(rg.empty_rig(rg.MAX_NODES)) and not _ok(rg.empty_rig(rg.MAX_NODES + 1)) and not _ok(rg.empty_rig(0))
    assert _ok(dict(rg.empty_rig(1), clips=[[]] * rg.MAX_CLIPS)) and not _ok(dict(rg.empty_rig(1), clips=[[]] * (rg.MAX_CLIPS + 1)))
    assert _ok(_with(("parent",), np.array([-1, 0, 1, 2], np.int32))) and _ok(_with(("parent",), np.array([-1, -1, -1, -1], np.int32)))
    for bad in ([-1, 1, 1, 0], [-1, 0, 2, 0], [0, 0, 1, 0], [-2, 0, 1, 0], [-1, 0, 1, 3], [-1, 0, 1, 4]):     # parent >= own index, < -1
        assert not _ok(_with(("parent",), np.array(bad, np.int32))), bad
    for name in ("translation", "rotation", "scale"):
        for bad in (np.nan, np.inf, -np.inf):
            assert not _ok(_with((name, (2, 1)), bad))
    assert _ok(_with(("translation", (2, 1)), 3e38)) and _ok(_with(("scale", (0, 0)), 0.0))
    for q, ok in (([0, 0, 0, 0.5], True), ([0, 0, 0, below(0.5)], False), ([0, 2, 0, 0], True), ([0, above(2.0), 0, 0], False), ([0, 0, 0, 0], False),
                  ([1, 1, 1, 1], True), ([1, 1, 1, above(1.0)], False), ([0.25, 0.25, 0.25, 0.25], True), ([0.25, 0.25, 0.25, below(0.25)], False)):
        assert _ok(_with(("rotation", 1), F(q))) == ok, q
        assert _ok(_with(("clips", 0, 1, "values", 1), F(q))) == ok, q    # the same rule for a rotation key
    # bindings
    assert not _ok(_with(("bindings", 0, "mesh"), 6)) and not _ok(_with(("bindings", 0, "mesh"), -1)) and _ok(_valid(), num_meshes=4, morphs={2: 2, 3: 4})
    assert not _ok(_with(("bindings", 0, "mesh"), 1))                     # bound twice
    assert not _ok(_with(("bindings", 0, "node"), 2))                     # both a node and joints
    assert _ok(_with(("bindings", 1, "node"), 0)) and not _ok(_with(("bindings", 1, "node"), 4)) and not _ok(_with(("bindings", 1, "node"), -2))
    assert _ok(_with(("bindings", 0, "joint_nodes"), np.array([3, 3, 3], np.uint16))) and not _ok(_with(("bindings", 0, "joint_nodes"), np.array([0, 4, 2], np.uint16)))
    assert not _ok(_valid(), skins={0: 2, 3: 2}) and not _ok(_valid(), skins={0: 4, 3: 2}) and not _ok(_valid(), skins={3: 2})     # other than the skin's; no skin
    assert not _ok(_valid(), morphs={1: 1, 2: 2, 3: 4})                   # a rigid binding of a morphed mesh
    assert not _ok(_valid(), morphs={3: 4})                               # mesh 2: neither node, joints nor morphs (and its WEIGHTS channel)
    assert not _ok(_with(("bindings", 1, "node"), -1))                    # mesh 1 likewise
    assert _ok(_with(("bindings", 3), dict(mesh=3)))                      # a skinned and morphed mesh bound by its weights alone
    assert _ok(_with(("bindings", 0), dict(mesh=0, node=2)))              # a skinned mesh bound rigidly
    for bad in (np.nan, np.inf):
        assert not _ok(_with(("bindings", 3, "inverse_bind", (1, 2, 3)), bad))
    assert _ok(_with(("bindings", 3, "inverse_bind", (1, 2, 3)), -3e38))
    # channels
    ch = ("clips", 0, 0)
    assert not _ok(_with(ch + ("path",), 4)) and not _ok(_with(ch + ("path",), -1)) and _ok(_with(ch + ("path",), rg.SCALE))
    assert not _ok(_with(ch + ("interpolation",), 2)) and not _ok(_with(ch + ("interpolation",), -1)) and _ok(_with(ch + ("interpolation",), rg.STEP))
    assert _ok(_with(ch + ("target",), 3)) and not _ok(_with(ch + ("target",), 4)) and not _ok(_with(ch + ("target",), -1))
    w = ("clips", 0, 3)
    assert not _ok(_with(w + ("target",), 6)) and not _ok(_with(w + ("target",), -1))
    assert not _ok(_with(w + ("target",), 5))                             # morphs, but not bound
    assert not _ok(_with(w + ("target",), 0))                             # bound, but no morphs
    assert not _ok(_with(w + ("target",), 4))                             # neither
    assert not _ok(_with(w + ("target",), 3))                             # (and mesh 3's weights would be there twice)
    assert not _ok(_with(ch + ("path",), rg.ROTATION))                    # node 1's rotation twice
    twice = _valid()
    twice["clips"][0].append(rg.channel(1, rg.TRANSLATION, [0], [[0, 0, 0]]))
    assert not _ok(twice)
    other_clip = _valid()
    other_clip["clips"][1].append(rg.channel(1, rg.TRANSLATION, [0], [[0, 0, 0]]))     # the same pair in another clip is another channel
    assert _ok(other_clip)
    assert not _ok(_with(ch, dict(target=1, path=rg.TRANSLATION, interpolation=rg.LINEAR, times=np.zeros(0, F), values=np.zeros((0, 3), F))))      # no keys
    assert not _ok(_with(ch, dict(rg.channel(1, rg.TRANSLATION, [0, 1], [[0, 0, 0], [1, 1, 1]]), values=np.zeros((2, 4), F))))
    for times, ok in (([0, 1], True), ([0, 0], False), ([1, 0], False), ([0, np.nextafter(F(0), F(1))], True), ([-1e30, 1e30], True),
                      ([0, np.nan], False), ([-np.inf, 0], False), ([0, np.inf], False)):
        assert _ok(_with(ch + ("times",), F(times))) == ok, times
    assert not _ok(_with(("clips", 0, 1, "times"), F([0, 2, 2]))) and not _ok(_with(("clips", 0, 1, "times"), F([0, 2, 1])))
    for bad in (np.nan, np.inf, -np.inf):
        assert not _ok(_with(ch + ("values", (1, 2)), bad)) and not _ok(_with(w + ("values", (0, 1)), bad))
    assert _ok(_with(ch + ("values", (1, 2)), -3e38))


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi_mirrors_match_the_header():
    fields = [("fovpt_rig_node", abi.RigNode, ("parent", "translation", "rotation", "scale")),
              ("fovpt_rig_binding", abi.RigBinding, ("mesh", "node", "num_joints", "_reserved", "joint_nodes", "inverse_bind")),
              ("fovpt_rig_channel", abi.RigChannel, ("target", "path", "interpolation", "num_keys", "times", "values")),
              ("fovpt_rig_clip", abi.RigClip, ("num_channels", "_reserved", "channels")),
              ("fovpt_rig_desc", abi.RigDesc, ("nodes", "num_nodes", "_reserved0", "bindings", "num_bindings", "_reserved1", "clips", "num_clips", "_reserved2"))]
    consts = ["FOVPT_RIG_MAX_NODES", "FOVPT_RIG_MAX_CLIPS", "FOVPT_RIG_MAX_KEYS", "FOVPT_RIG_TRANSLATION", "FOVPT_RIG_ROTATION", "FOVPT_RIG_SCALE",
              "FOVPT_RIG_WEIGHTS", "FOVPT_RIG_STEP", "FOVPT_RIG_LINEAR"]
    lays, values = header_layout.probe([(cname, names) for cname, _, names in fields], consts)
    got = [x for lay in lays for x in lay] + values
    want = []
    for _, S, names in fields:
        want += [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names]
    want += [abi.RIG_MAX_NODES, abi.RIG_MAX_CLIPS, abi.RIG_MAX_KEYS, abi.RIG_TRANSLATION, abi.RIG_ROTATION, abi.RIG_SCALE, abi.RIG_WEIGHTS,
             abi.RIG_STEP, abi.RIG_LINEAR]
    assert got == want
    sizes = [ctypes.sizeof(S) for _, S, _ in fields]
    assert sizes == [44, 32, 32, 16, 48]
    assert (rg.MAX_NODES, rg.MAX_CLIPS, rg.MAX_KEYS) == (1024, 64, 1 << 20) == (abi.RIG_MAX_NODES, abi.RIG_MAX_CLIPS, abi.RIG_MAX_KEYS)
    assert (rg.TRANSLATION, rg.ROTATION, rg.SCALE, rg.WEIGHTS, rg.STEP, rg.LINEAR) == (0, 1, 2, 3, 0, 1)
