"""numpy float32 restatement of fovpt_update_morphed (csrc/refit.hip, k_morph_vertices / k_morph_skin_vertices), the overflow
rules of its validation, and the procedural targets and weights the tests share.

A mesh has targets t = 0, 1, ...; a target lists some of the mesh's vertices, each with a delta d.  A pose gives one weight per
target.  With p = (x, y, z) a vertex's REST position (the one fovpt_set_scene received), walk the targets in ascending order; for
every target that lists the vertex and whose weight has w[t] != 0.0f

    p.x = p.x + w[t] * d.x          p.y, p.z likewise

every * and + one binary32 operation, none fused.  A weight of +0 or -0 skips its target: nothing is added, so a coordinate of
-0 stays -0.  With a palette the morphed p then goes through skin_ref.apply with the mesh's skin.  numpy's float32 arrays round
after every operation, so the expressions below are that arithmetic as written.

A target is written as the python wrapper's set_morphs takes it: a dense (n, 3) array of deltas, or a pair (index (k,) strictly
ascending, delta (k, 3))."""
import numpy as np

import skin_ref as sk

F = np.float32
LIMIT = 2.0 ** 127
MAX_TARGETS = 256


def split(target, n):
    """(index (k,) int64, delta (k, 3) float32) of a dense or sparse target of a mesh of n vertices."""
    if isinstance(target, tuple):
        idx, d = np.asarray(target[0]).astype(np.int64).reshape(-1), np.asarray(target[1], F).reshape(-1, 3)
        assert idx.shape[0] == d.shape[0] and (np.diff(idx) > 0).all() and (idx.size == 0 or (idx[0] >= 0 and idx[-1] < n))
        return idx, d
    d = np.asarray(target, F)
    assert d.shape == (n, 3)
    return np.arange(n, dtype=np.int64), d


def apply(rest, targets, weights):
    """rest (n, 3) float32, targets a list, weights one per target -> (n, 3) float32."""
    p = np.array(rest, F).reshape(-1, 3)
    w = np.asarray(weights, F).reshape(-1)
    assert w.shape[0] == len(targets)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for t, target in enumerate(targets):
            if not w[t] != F(0):                                          # +0 and -0: skipped, not applied
                continue
            idx, d = split(target, p.shape[0])
            prod = w[t] * d
            assert prod.dtype == F
            p[idx] = p[idx] + prod                                        # (a target lists a vertex once)
    return p


def apply_skinned(rest, targets, weights, joints, skin_weights, pal):
    """The morphed positions through skin_ref.apply: fovpt_update_morphed with matrices."""
    return sk.apply(apply(rest, targets, weights), joints, skin_weights, pal)


def target_max(targets, n):
    """D: per target the largest |delta component| in binary64, 0 for an empty target."""
    return np.array([np.abs(split(t, n)[1].astype(np.float64)).max() if split(t, n)[1].size else 0.0 for t in targets], np.float64)


def bound(rest, targets, weights):
    """B = A + sum over ascending t of |w[t]| D[t] in binary64, A the largest |coordinate| of rest.  A morphed coordinate is, in
    exact arithmetic, rest's plus some of the w[t] d: every partial sum, and every product alone, is within B.  Below 2^127 the
    other half of the binary32 range absorbs the roundings (at most 2 x 256 operations, each within 2^-24 relative)."""
    rest = np.asarray(rest, np.float64).reshape(-1, 3)
    b = float(np.abs(rest).max()) if rest.size else 0.0
    for wt, d in zip(np.asarray(weights, F).reshape(-1).astype(np.float64), target_max(targets, rest.shape[0])):
        b = b + abs(wt) * d
    return b


def row_bound(rest, targets, weights, skin_weights, pal):
    """skin_ref.overflow_bound with B in A's place: the largest S ((|m0| + |m1| + |m2|) B + |m3|) over the palette's rows."""
    P = np.abs(sk.palette(pal).astype(np.float64)).reshape(-1, 4)
    return float((sk.weight_sum(skin_weights) * (((P[:, 0] + P[:, 1]) + P[:, 2]) * bound(rest, targets, weights) + P[:, 3])).max())


def entry_bound(skin_weights, pal):
    """The largest S |m| over the first three columns of the palette (the entries of the blended matrix that row_bound covers
    only when B >= 1)."""
    return float(sk.weight_sum(skin_weights) * np.abs(sk.palette(pal).astype(np.float64)).reshape(-1, 4)[:, :3].max())


def accepted(rest, targets, weights, skin_weights=None, pal=None):
    """fovpt_update_morphed's rule for host data: finite weights and B <= 2^127; with a palette also finite entries, no row
    above 2^127 with B in A's place and no entry of the first three columns above 2^127 / S."""
    if not np.isfinite(np.asarray(weights, F)).all() or bound(rest, targets, weights) > LIMIT:
        return False
    if pal is None:
        return True
    return bool(np.isfinite(sk.palette(pal)).all() and not row_bound(rest, targets, weights, skin_weights, pal) > LIMIT
                and not entry_bound(skin_weights, pal) > LIMIT)


def restate(model, morphs, poses, skins=None):
    """{mesh: positions} of fovpt_update_morphed(poses) on model with morphs {mesh: targets}: poses maps a mesh to its weights
    or to (weights, palette), the latter with skins {mesh: (joints, weights, ...)}.  What fovpt_update_vertices is given
    instead."""
    out = {}
    for k, p in poses.items():
        v = model.meshes[k].vertex
        if isinstance(p, tuple):
            out[k] = apply_skinned(v, morphs[k], p[0], skins[k][0], skins[k][1], p[1])
        else:
            out[k] = apply(v, morphs[k], p)
    return out


# ---- targets and weights the tests share ---------------------------------------------------------------------------------------
def random_targets(rng, n, num_targets, dense=0, fraction=0.3, scale=4.0):
    """num_targets targets for n vertices: the first `dense` of them dense, the others sparse over about `fraction` of the
    vertices (sometimes none); deltas up to `scale`, with exact zeros among them."""
    out = []
    for t in range(num_targets):
        if t < dense:
            idx = np.arange(n)
        else:
            idx = np.flatnonzero(rng.uniform(0, 1, n) < (0.0 if rng.uniform() < 0.1 else fraction))
        d = (rng.uniform(-scale, scale, (len(idx), 3)) * (rng.uniform(0, 1, (len(idx), 3)) < 0.9)).astype(F)
        out.append(d if t < dense else (idx.astype(np.uint32), d))
    return out


def random_weights(rng, num_targets, active=0.5):
    """One weight per target: exact zeros of either sign, negatives and values above 1 among them."""
    w = rng.uniform(-1.5, 2.5, num_targets)
    off = rng.uniform(0, 1, num_targets) >= active
    w = np.where(off, np.where(rng.uniform(0, 1, num_targets) < 0.5, 0.0, -0.0), w)
    return w.astype(F)


def bumps(vertex, num_dense, num_sparse, fraction=0.05, height=None):
    """Procedural targets for a mesh of any shape: num_dense dense targets (low-frequency waves along the axes) and num_sparse
    sparse ones, each a bump over the `fraction` of the vertices nearest to one of the mesh's vertices.  height: the largest
    displacement (default: 5 % of the mesh's extent)."""
    v = np.asarray(vertex, np.float64).reshape(-1, 3)
    n = v.shape[0]
    ext = float(np.ptp(v, axis=0).max()) if n else 1.0
    h = (0.05 * ext if height is None else height) or 1.0
    out = []
    for t in range(num_dense):
        ph = (v[:, (t + 1) % 3] - v[:, (t + 1) % 3].min()) / (ext or 1.0) * (1 + t // 3) * np.pi
        d = np.zeros((n, 3))
        d[:, t % 3] = h * np.sin(ph)
        out.append(d.astype(F))
    k = max(1, int(round(fraction * n))) if n else 0
    for t in range(num_sparse):
        if n == 0:
            out.append((np.zeros(0, np.uint32), np.zeros((0, 3), F)))
            continue
        c = v[(t * 7919) % n]
        dist = np.linalg.norm(v - c, axis=1)
        idx = np.sort(np.argpartition(dist, k - 1)[:k])
        fall = 1.0 - dist[idx] / (dist[idx].max() or 1.0)
        d = np.zeros((k, 3))
        d[:, t % 3] = h * (0.25 + 0.75 * fall)
        out.append((idx.astype(np.uint32), d.astype(F)))
    return out
