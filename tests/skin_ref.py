"""numpy float32 restatement of fovpt_update_skinned (csrc/refit.hip, k_skin_vertices), the overflow rule of its validation, and
the procedural skins and poses the tests share.

A skin gives every vertex of a mesh four joint indices j0 .. j3 and four weights w0 .. w3; a pose is the mesh's palette J of
row-major 3 x 4 matrices.  With (x, y, z) the vertex's REST position (the one fovpt_set_scene received), entry e = 0 .. 11 of the
blended matrix is

    M[e] = ((w0 * J[j0][e] + w1 * J[j1][e]) + w2 * J[j2][e]) + w3 * J[j3][e]
    x'   = ((M[0] * x + M[1] * y) + M[2] * z) + M[3]          y', z': rows 1 and 2

every * and + one binary32 operation, none fused; the weights are used as given, not normalised.  numpy's float32 arrays round
after every operation, so the expressions below are that arithmetic as written."""
import numpy as np

import transform_ref as tf

F = np.float32
LIMIT = 2.0 ** 127
MAX_JOINTS = 1024


def palette(p):
    """(J, 12) float32 from a (J, 3, 4), (J, 4, 4) (last rows 0 0 0 1) or (J, 12) palette."""
    p = np.asarray(p, F)
    if p.ndim == 3 and p.shape[1:] == (4, 4):
        assert (p[:, 3] == F([0, 0, 0, 1])).all()
        p = p[:, :3]
    return np.ascontiguousarray(p.reshape(-1, 12))


def apply(rest, joints, weights, pal):
    """rest (n, 3) float32, joints (n, 4) integers, weights (n, 4) float32, pal a palette -> (n, 3) float32."""
    rest, P = np.asarray(rest, F).reshape(-1, 3), palette(pal)
    j, w = np.asarray(joints).reshape(-1, 4).astype(np.int64), np.asarray(weights, F).reshape(-1, 4)
    assert j.shape[0] == w.shape[0] == rest.shape[0] and (j >= 0).all() and (j < P.shape[0]).all()
    x, y, z = rest[:, 0], rest[:, 1], rest[:, 2]
    out = np.empty_like(rest)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        M = ((w[:, 0:1] * P[j[:, 0]] + w[:, 1:2] * P[j[:, 1]]) + w[:, 2:3] * P[j[:, 2]]) + w[:, 3:4] * P[j[:, 3]]
        assert M.dtype == F
        for r in range(3):
            out[:, r] = ((M[:, 4 * r] * x + M[:, 4 * r + 1] * y) + M[:, 4 * r + 2] * z) + M[:, 4 * r + 3]
    return out


def weight_sum(weights):
    """S: the largest ((w0 + w1) + w2) + w3 over the vertices, in binary64 (0 for a mesh without vertices)."""
    w = np.asarray(weights, F).reshape(-1, 4).astype(np.float64)
    return float((((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]).max()) if w.size else 0.0


def overflow_bound(rest, weights, pal):
    """The largest S * ((|m0| + |m1| + |m2|) * A + |m3|) over the rows of the palette's matrices, in binary64: A the largest
    |coordinate| of rest, S weight_sum(weights).  With B the largest (|m0| + |m1| + |m2|) A + |m3| of the palette, every partial
    sum of a blended row applied to a vertex is, in exact arithmetic, a sum of terms w_k |J[j_k][c]| |coordinate| and
    w_k |J[j_k][3]| over some of the joints and columns: at most sum_k w_k B <= S B.  Below 2^127 the other half of the binary32
    range absorbs the roundings (two dozen operations, each within 2^-24 relative).  With S = 1 this is
    transform_ref.overflow_bound."""
    rest, P = np.asarray(rest, np.float64).reshape(-1, 3), np.abs(palette(pal).astype(np.float64)).reshape(-1, 4)
    a = np.abs(rest).max() if rest.size else 0.0
    return float((weight_sum(weights) * (((P[:, 0] + P[:, 1]) + P[:, 2]) * a + P[:, 3])).max())


def entry_bound(weights, pal):
    """The largest S * |m| over the entries of the palette, in binary64.  The library computes the blended matrix first, and an
    entry of it is a sum of w_k J[j_k][e]: at most S max |J[.][e]|, which overflow_bound covers for the fourth column always
    and for the others only when A >= 1.  This closes the case A < 1."""
    return float(weight_sum(weights) * np.abs(palette(pal).astype(np.float64)).max())


def accepted(rest, weights, pal):
    """fovpt_update_skinned's rule for host matrices: finite entries, no row above 2^127 and no entry above 2^127 / S."""
    return bool(np.isfinite(palette(pal)).all() and not overflow_bound(rest, weights, pal) > LIMIT and not entry_bound(weights, pal) > LIMIT)


def restate(model, skins, poses):
    """{mesh: positions} of fovpt_update_skinned({mesh: palette}) on model with skins {mesh: (joints, weights, ...)}: what
    fovpt_update_vertices is given instead."""
    return {k: apply(model.meshes[k].vertex, skins[k][0], skins[k][1], p) for k, p in poses.items()}


# ---- skins and poses the tests share (built in binary64, rounded once to binary32) ---------------------------------------------
def bend(vertex, n_joints):
    """(joints (n, 4) uint16, weights (n, 4) float32, n_joints): n_joints joints stacked at equal steps along the mesh's tallest
    axis, every vertex weighted between the two it lies between (one joint: weight 1 on it); the third and fourth slots have
    weight 0 and index 0, and so has the second slot where the vertex sits exactly on a joint."""
    v = np.asarray(vertex, np.float64).reshape(-1, 3)
    n = v.shape[0]
    j, w = np.zeros((n, 4), np.uint16), np.zeros((n, 4), F)
    if n_joints == 1 or n == 0:
        w[:, 0] = 1
        return j, w, n_joints
    ext = v.max(axis=0) - v.min(axis=0)
    ax = int(np.argmax(ext))
    s = (v[:, ax] - v[:, ax].min()) / (ext[ax] if ext[ax] > 0 else 1.0) * (n_joints - 1)
    a = np.minimum(np.floor(s), n_joints - 2)
    t = (s - a).astype(F)
    j[:, 0], j[:, 1] = a, a + 1
    w[:, 0], w[:, 1] = (1.0 - (s - a)).astype(F), t
    low = t == 0                                                          # exactly on joint a
    j[low, 1] = 0
    return j, w, n_joints


def bend_pose(vertex, n_joints, deg, t):
    """(n_joints, 3, 4): joint k turned by deg (k + 1) / n_joints about the vertical axis through the mesh's centre and carried
    by t (k + 1) / n_joints."""
    c = np.asarray(vertex, np.float64).reshape(-1, 3).mean(axis=0) if len(vertex) else np.zeros(3)
    t = np.asarray(t, np.float64)
    return np.stack([tf.rotation_translation(deg * (k + 1) / n_joints, c, t * (k + 1) / n_joints) for k in range(n_joints)])


def dense_matrix(centre=(368.0, 0.0, 351.0)):
    """A (3, 4) turn and carry with a small shear added: no entry is zero."""
    m = tf.rotation_translation(23.0, centre, (-40.0, 12.0, -30.0)).astype(np.float64)
    m[:, :3] += np.array([[0.0, 0.03125, 0.0], [0.015625, 0.0, -0.0625], [0.0, 0.046875, 0.0]])
    m = m.astype(F)
    assert (m != 0).all()
    return m


def random_skin(rng, n, n_joints):
    """(joints, weights, n_joints) for n vertices: any joint in any slot, weights with exact zeros; half of the rows are scaled to
    sum to about 1, the others are left as drawn (sums anywhere in 0 .. 4)."""
    j = rng.integers(0, n_joints, (n, 4)).astype(np.uint16)
    w = rng.uniform(0.0, 1.0, (n, 4)) * (rng.uniform(0, 1, (n, 4)) < 0.7)
    s = w.sum(axis=1, keepdims=True)
    unit = (rng.uniform(0, 1, (n, 1)) < 0.5) & (s > 0)
    w = np.where(unit, w / np.where(s > 0, s, 1.0), w).astype(F)
    return j, np.minimum(w, F(1)), n_joints


def random_pose(rng, vertex, n_joints):
    """(n_joints, 3, 4): per joint a turn about the mesh's centre and a carry, every other one also scaled unevenly."""
    c = np.asarray(vertex, np.float64).reshape(-1, 3).mean(axis=0)
    out = []
    for k in range(n_joints):
        m = tf.rotation_translation(rng.uniform(-40, 40), c, rng.uniform(-5, 5, 3)).astype(np.float64)
        if k % 2:
            s = tf.scale_about(c, rng.uniform(0.6, 1.4, 3)).astype(np.float64)
            m = np.concatenate([m[:, :3] @ s[:, :3], (m[:, :3] @ s[:, 3] + m[:, 3])[:, None]], axis=1)
        out.append(m.astype(F))
    return np.stack(out)
