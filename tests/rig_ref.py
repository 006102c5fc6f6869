"""numpy float32 restatement of fovpt_set_rig / fovpt_update_animated (csrc/rig.hip, k_rig_pose): the definition in include/fovpt.h
operation by operation, the validation rules, and the procedural rigs the tests share.

A rig is a dict (renderer.SampleRenderer.pack_rig's form): parent (N,), translation (N, 3), rotation (N, 4) as x y z w, scale
(N, 3); bindings, a list of dicts with mesh and node, or joint_nodes (J,) and inverse_bind (J, 3, 4), or neither; clips, a list
of lists of channels, each a dict with target, path, interpolation, times (K,) and values (K, width).

Every *, +, -, / and square root below is one binary32 operation: the operands are numpy float32 scalars or arrays, which round
after every operation (constants are written F(...): a bare Python float would widen a scalar expression).  Sine and arc cosine
are the library's deterministic ones through oracle.math_op, as expose_ref.py takes its pow."""
import numpy as np

import morph_ref as mr
import skin_ref as sk
import transform_ref as tf

F = np.float32
MAX_NODES, MAX_CLIPS, MAX_KEYS = 1024, 64, 1 << 20
TRANSLATION, ROTATION, SCALE, WEIGHTS = 0, 1, 2, 3
STEP, LINEAR = 0, 1
OP_SIN, OP_ACOS = 1, 3                  # FOVPT_OP_SIN, FOVPT_OP_ACOS
SLERP_LINEAR_ABOVE = F(0.9995)


def _sin(oracle, x):
    return oracle.math_op(OP_SIN, np.array([x], F))[0]


def _acos(oracle, x):
    return oracle.math_op(OP_ACOS, np.array([x], F))[0]


# ---- step 1: sampling -------------------------------------------------------------------------------------------------------
def locate(times, T):
    """(k, u): u None when key k is used as given (T before the first key, behind the last), else the segment's first key and
    u = (T - t_k) / (t_{k+1} - t_k) in binary32."""
    t, T = np.asarray(times, F), F(T)
    n = t.shape[0]
    if T <= t[0]:
        return 0, None
    if T >= t[n - 1]:
        return n - 1, None
    k = int(np.searchsorted(t, T, side="right")) - 1                      # the largest k with t_k <= T
    return k, (T - t[k]) / (t[k + 1] - t[k])


def slerp(oracle, a, b, u):
    a, b, u = np.asarray(a, F), np.asarray(b, F), F(u)
    d = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]
    if d < 0:
        b, d = -b, -d
    if d > SLERP_LINEAR_ABOVE:
        q = a + u * (b - a)
    else:
        th = _acos(oracle, d)
        s = _sin(oracle, th)
        wa = _sin(oracle, (F(1.0) - u) * th) / s
        wb = _sin(oracle, u * th) / s
        q = wa * a + wb * b
    n = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    assert q.dtype == F and n.dtype == F
    return q / n


def sample(oracle, channel, T):
    """The channel's value at T: (width,) float32."""
    v = np.asarray(channel["values"], F)
    v = v.reshape(len(channel["times"]), -1)
    k, u = locate(channel["times"], T)
    if u is None or channel["interpolation"] == STEP:
        return v[k].copy()                                                # as given, not normalised
    if channel["path"] == ROTATION:
        return slerp(oracle, v[k], v[k + 1], u)
    return v[k] + u * (v[k + 1] - v[k])


# ---- steps 2 to 4: local, world, palette ----------------------------------------------------------------------------------
def local(t, q, s):
    """(3, 4) float32 from translation, rotation x y z w and scale."""
    t, s = np.asarray(t, F), np.asarray(s, F)
    x, y, z, w = [F(c) for c in q]
    one, two = F(1.0), F(2.0)
    r = np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                  [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                  [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], F)
    return np.concatenate([r * s[None, :], t[:, None]], axis=1)


def compose(P, L):
    """P o L of two (3, 4) float32 matrices."""
    P, L = np.asarray(P, F).reshape(3, 4), np.asarray(L, F).reshape(3, 4)
    out = np.empty((3, 4), F)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        out[:, :3] = (P[:, 0:1] * L[0:1, :3] + P[:, 1:2] * L[1:2, :3]) + P[:, 2:3] * L[2:3, :3]
        out[:, 3] = ((P[:, 0] * L[0, 3] + P[:, 1] * L[1, 3]) + P[:, 2] * L[2, 3]) + P[:, 3]
    return out


def pose(oracle, rig, clip, T, morphs=None):
    """The clip at T -> dict(world (N, 3, 4), palettes: per binding with joints its (J, 3, 4) in binding order, rigid: per rigid
    binding its (3, 4) in binding order, weights {mesh: (targets,)} for the bound meshes of morphs {mesh: target count})."""
    T = F(T)
    n = len(rig["parent"])
    trs = [np.array(rig[k], F).reshape(n, -1) for k in ("translation", "rotation", "scale")]
    wch = {}
    for ch in rig["clips"][clip]:
        if ch["path"] == WEIGHTS:
            wch[int(ch["target"])] = ch
        else:
            trs[ch["path"]][int(ch["target"])] = sample(oracle, ch, T)
    world = np.empty((n, 3, 4), F)
    for i in range(n):
        L = local(trs[0][i], trs[1][i], trs[2][i])
        p = int(rig["parent"][i])
        world[i] = L if p < 0 else compose(world[p], L)
    palettes, rigid, weights = [], [], {}
    for b in rig.get("bindings", ()):
        if b.get("joint_nodes") is not None:
            ib = sk.palette(b["inverse_bind"]).reshape(-1, 3, 4)
            palettes.append(np.stack([compose(world[int(j)], ib[k]) for k, j in enumerate(b["joint_nodes"])]))
        elif b.get("node", -1) >= 0:
            rigid.append(world[int(b["node"])].copy())
        nt = (morphs or {}).get(b["mesh"], 0)
        if nt:
            weights[b["mesh"]] = sample(oracle, wch[b["mesh"]], T) if b["mesh"] in wch else np.zeros(nt, F)
    return dict(world=world, palettes=palettes, rigid=rigid, weights=weights)


def drives(oracle, rig, clip, T, morphs=None):
    """What fovpt_update_animated hands to the other update calls: (skinned {mesh: palette}, morphed {mesh: weights or (weights,
    palette)}, rigid {mesh: matrix}); morphs {mesh: targets}."""
    P = pose(oracle, rig, clip, T, {k: len(v) for k, v in (morphs or {}).items()})
    skinned, morphed, rigid = {}, {}, {}
    pals, rig_m = iter(P["palettes"]), iter(P["rigid"])
    for b in rig.get("bindings", ()):
        m = b["mesh"]
        pal = next(pals) if b.get("joint_nodes") is not None else None
        if m in P["weights"]:
            morphed[m] = P["weights"][m] if pal is None else (P["weights"][m], pal)
        elif pal is not None:
            skinned[m] = pal
        else:
            rigid[m] = next(rig_m)
    return skinned, morphed, rigid


def restate(oracle, model, rig, clip, T, skins=None, morphs=None):
    """{mesh: positions} of fovpt_update_animated(clip, T) on model with skins {mesh: (joints, weights, ...)} and morphs {mesh:
    targets}: what fovpt_update_vertices is given instead."""
    skinned, morphed, rigid = drives(oracle, rig, clip, T, morphs)
    out = sk.restate(model, skins or {}, skinned)
    out.update(mr.restate(model, morphs or {}, morphed, skins))
    out.update(tf.restate(model, rigid))
    return out


# ---- fovpt_set_rig's rules -----------------------------------------------------------------------------------------------------
def norm2_ok(q):
    """The squared norm in binary64 within [1/4, 4]."""
    x, y, z, w = [float(F(c)) for c in q]
    return 0.25 <= ((x * x + y * y) + z * z) + w * w <= 4.0


def accepted(rig, num_meshes, skins=None, morphs=None):
    """fovpt_set_rig's rules for a rig of this module's form (the null pointers and reserved fields of the C structs aside):
    skins {mesh: joint count}, morphs {mesh: target count} of the scene."""
    skins, morphs = skins or {}, morphs or {}
    parent = np.asarray(rig["parent"])
    n = parent.shape[0]
    if not 1 <= n <= MAX_NODES or len(rig.get("clips", ())) > MAX_CLIPS:
        return False
    if any(int(p) < -1 or int(p) >= i for i, p in enumerate(parent)):
        return False
    rest = [np.asarray(rig[k], F).reshape(n, -1) for k in ("translation", "rotation", "scale")]
    if not all(np.isfinite(a).all() for a in rest) or not all(norm2_ok(q) for q in rest[1]):
        return False
    bound = set()
    for b in rig.get("bindings", ()):
        m, node = int(b["mesh"]), int(b.get("node", -1))
        jn = b.get("joint_nodes")
        nj = 0 if jn is None else len(jn)
        if not 0 <= m < num_meshes or m in bound or not -1 <= node < n or (node >= 0 and nj):
            return False
        bound.add(m)
        if nj and (nj != skins.get(m, 0) or any(not 0 <= int(j) < n for j in jn)):
            return False
        if (node >= 0 and morphs.get(m, 0)) or (node < 0 and not nj and not morphs.get(m, 0)):
            return False
        if nj and (sk.palette(b["inverse_bind"]).shape[0] != nj or not np.isfinite(sk.palette(b["inverse_bind"])).all()):
            return False
    for clip in rig.get("clips", ()):
        seen = set()
        for ch in clip:
            path, target = int(ch["path"]), int(ch["target"])
            if path not in (TRANSLATION, ROTATION, SCALE, WEIGHTS) or ch["interpolation"] not in (STEP, LINEAR):
                return False
            if path == WEIGHTS:
                if not 0 <= target < num_meshes or target not in bound or not morphs.get(target, 0):
                    return False
                width = morphs[target]
            else:
                if not 0 <= target < n:
                    return False
                width = 4 if path == ROTATION else 3
            if (target, path) in seen:
                return False
            seen.add((target, path))
            t, v = np.asarray(ch["times"], F), np.asarray(ch["values"], F)
            if not 1 <= t.shape[0] <= MAX_KEYS or v.size != width * t.shape[0]:
                return False
            if not np.isfinite(t).all() or not (np.diff(t.astype(np.float64)) > 0).all() or not np.isfinite(v).all():
                return False
            if path == ROTATION and not all(norm2_ok(q) for q in v.reshape(-1, 4)):
                return False
    return True


# ---- rigs the tests share (built in binary64, rounded once to binary32) ------------------------------------------------------
def quat(axis, deg, norm=1.0):
    """x y z w of a turn by deg about axis, scaled to the given norm."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = np.deg2rad(deg) / 2.0
    return (np.concatenate([a * np.sin(h), [np.cos(h)]]) * norm).astype(F)


def channel(target, path, times, values, interpolation=LINEAR):
    t = np.asarray(times, F)
    return dict(target=int(target), path=int(path), interpolation=int(interpolation), times=t, values=np.asarray(values, F).reshape(t.shape[0], -1))


def empty_rig(n):
    """n roots at the identity, no bindings, one empty clip."""
    return dict(parent=np.full(n, -1, np.int32), translation=np.zeros((n, 3), F), rotation=np.tile(F([0, 0, 0, 1]), (n, 1)),
                scale=np.ones((n, 3), F), bindings=[], clips=[[]])


def inverse_bind_of(rig, nodes):
    """(J, 3, 4): the inverses of the nodes' rest worlds (binary64, rounded once), so that the rest pose leaves a mesh about
    where it is."""
    n = len(rig["parent"])
    W = np.empty((n, 4, 4))
    for i in range(n):
        x, y, z, w = np.asarray(rig["rotation"][i], np.float64)
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        L = np.eye(4)
        L[:3, :3] = R * np.asarray(rig["scale"][i], np.float64)[None, :]
        L[:3, 3] = rig["translation"][i]
        p = int(rig["parent"][i])
        W[i] = L if p < 0 else W[p] @ L
    return np.stack([np.linalg.inv(W[int(j)])[:3] for j in nodes]).astype(F)


def random_rig(rng, n, max_depth=None, scales=True, clip_channels=0.6, chains=0.0):
    """n nodes, every parent drawn below the node's own index (within max_depth levels; with probability `chains` the node
    before it, which makes long chains), rest poses of turns, carries and, with
    scales, uneven scales; one clip with a channel of 1 to 4 keys on about clip_channels of the (node, path) pairs: STEP and
    LINEAR, rotation keys near each other and far apart (both slerp branches), some of them not unit."""
    rig = empty_rig(n)
    depth = np.zeros(n, np.int64)
    for i in range(1, n):
        ok = [p for p in range(i) if max_depth is None or depth[p] + 1 < max_depth]
        p = int(rng.choice(ok)) if ok and rng.uniform() < 0.9 else -1
        if ok and ok[-1] == i - 1 and rng.uniform() < chains:
            p = i - 1
        rig["parent"][i] = p
        depth[i] = 0 if p < 0 else depth[p] + 1
    for i in range(n):
        rig["translation"][i] = rng.uniform(-3, 3, 3)
        rig["rotation"][i] = quat(rng.standard_normal(3), rng.uniform(-170, 170))
        if scales:
            rig["scale"][i] = rng.uniform(0.7, 1.3, 3)
    clip = []
    for i in range(n):
        for path in (TRANSLATION, ROTATION, SCALE):
            if rng.uniform() > clip_channels or (path == SCALE and not scales):
                continue
            k = int(rng.integers(1, 5))
            times = np.cumsum(rng.uniform(0.1, 1.0, k)).astype(F)
            if path == ROTATION:
                base = quat(rng.standard_normal(3), rng.uniform(-170, 170))
                vals = [base]
                for _ in range(k - 1):
                    step = rng.choice([1.0, 3.0, 60.0, 150.0])           # d above 0.9995, below it, and negative
                    dq = quat(rng.standard_normal(3), step)
                    x1, y1, z1, w1 = vals[-1].astype(np.float64)
                    x2, y2, z2, w2 = dq.astype(np.float64)
                    nxt = np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                                    w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])
                    vals.append((nxt * rng.choice([1.0, -1.0]) * (rng.uniform(0.8, 1.25) if scales else 1.0)).astype(F))
                vals = np.stack(vals)
            elif path == TRANSLATION:
                vals = rng.uniform(-3, 3, (k, 3))
            else:
                vals = rng.uniform(0.7, 1.3, (k, 3))
            clip.append(channel(i, path, times, vals, STEP if rng.uniform() < 0.2 else LINEAR))
    rig["clips"] = [clip]
    return rig


def flat_rig(n):
    """n roots, each turning and travelling on its own: one level."""
    rig = empty_rig(n)
    k = np.arange(n, dtype=np.float64)
    rig["translation"] = np.stack([np.cos(k), 0.01 * k, np.sin(k)], axis=1).astype(F)
    rig["clips"] = [[channel(i, ROTATION, [0.0, 1.0], [quat((0, 1, 0), 0.0), quat((0.2, 1, 0.1), 20.0 + i % 97)]) for i in range(0, n, 3)] +
                    [channel(i, TRANSLATION, [0.25, 0.75], [[0, 0, 0], [i % 5, 1, -2]]) for i in range(1, n, 3)]]
    return rig


def chain_rig(n):
    """One chain of n nodes, each a small carry and a small turn on its parent: as many levels as nodes.  (Turns of about 90 / n
    degrees: the last node is a quarter turn from the first.)"""
    rig = empty_rig(n)
    rig["parent"] = np.arange(-1, n - 1, dtype=np.int32)
    rig["translation"][:] = F([0.0, 1.0 / n, 0.0])
    a = 90.0 / n
    rig["clips"] = [[channel(i, ROTATION, [0.0, 1.0], [quat((0, 0, 1), 0.0), quat((0.1, 0.0, 1.0), a * (1 + (i % 3)))]) for i in range(n)]]
    return rig
