"""numpy float32 restatement of fovpt_update_transforms (csrc/refit.hip, k_transform_vertices), the overflow rule of its
validation, and the tolerance the device's hierarchy cost (fovpt_hierarchy_cost) is compared with refit_ref.sah_cost under.

A transform is a row-major 3 x 4 matrix m applied to a mesh's REST positions (the ones fovpt_set_scene received):

    x' = ((m[0] * x + m[1] * y) + m[2] * z) + m[3]          y', z': rows 1 and 2

every * and + one binary32 operation, none fused.  numpy's float32 arrays round after every operation, so the expression below
is that arithmetic as written."""
import numpy as np

F = np.float32
LIMIT = 2.0 ** 127


def matrix(m):
    """(3, 4) float32 from a (3, 4), (4, 4) (last row 0 0 0 1) or flat 12-entry matrix."""
    m = np.asarray(m, F)
    if m.shape == (4, 4):
        assert np.array_equal(m[3], F([0, 0, 0, 1]))
        m = m[:3]
    return np.ascontiguousarray(m.reshape(3, 4))


def apply(rest, m):
    """rest (n, 3) float32, m a matrix -> (n, 3) float32."""
    rest, m = np.asarray(rest, F).reshape(-1, 3), matrix(m)
    x, y, z = rest[:, 0], rest[:, 1], rest[:, 2]
    out = np.empty_like(rest)
    with np.errstate(over="ignore", under="ignore"):
        for r in range(3):
            out[:, r] = ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]
    return out


def overflow_bound(rest, m):
    """The largest (|m0| + |m1| + |m2|) * A + |m3| over the rows, in binary64, A the largest |coordinate| of rest (0 for a mesh
    without vertices).  Every partial sum of a row is bounded by it in magnitude, so below 2^127 (half the largest binary32
    power of two: room for the roundings) no intermediate value overflows."""
    rest, m = np.asarray(rest, np.float64).reshape(-1, 3), matrix(m).astype(np.float64)
    a = np.abs(rest).max() if rest.size else 0.0
    return float((np.abs(m[:, :3]).sum(axis=1) * a + np.abs(m[:, 3])).max())


def accepted(rest, m):
    """fovpt_update_transforms' rule: finite entries and no row above 2^127."""
    return bool(np.isfinite(matrix(m)).all() and not overflow_bound(rest, m) > LIMIT)


def restate(model, transforms):
    """{mesh: positions} of fovpt_update_transforms({mesh: matrix}) on model: what fovpt_update_vertices is given instead."""
    return {k: apply(model.meshes[k].vertex, m) for k, m in transforms.items()}


# ---- matrices the tests share (built in binary64, rounded once to binary32) ---------------------------------------------------
def rotation_translation(deg, axis_point, t):
    """A turn by deg about the vertical axis through axis_point, then the translation t."""
    a = np.deg2rad(deg)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    c = np.asarray(axis_point, np.float64)
    return np.concatenate([R, (c - R @ c + np.asarray(t, np.float64))[:, None]], axis=1).astype(F)


def scale_about(centre, s):
    c, s = np.asarray(centre, np.float64), np.asarray(s, np.float64)
    return np.concatenate([np.diag(s), (c - s * c)[:, None]], axis=1).astype(F)


def collapse_to(point):
    """The singular matrix that sends every vertex to point."""
    return np.concatenate([np.zeros((3, 3)), np.asarray(point, np.float64)[:, None]], axis=1).astype(F)


IDENTITY = np.eye(3, 4, dtype=F)


# ---- the hierarchy cost --------------------------------------------------------------------------------------------------------
def live_entries(nodes, levels):
    """The child entries of the first levels[-1] wide nodes (uint32 (N, 32)) that are not empty slots."""
    nf = np.asarray(nodes, np.uint32).reshape(-1, 32).view(F).reshape(-1, 4, 8)[:levels[-1]]
    return int((nf[:, :, 0] < np.inf).sum())


def cost_tolerance(entries):
    """Relative tolerance between two binary64 evaluations of refit_ref.sah_cost's expression that differ in summation order
    only: (E + 16) 2^-52, E the live entries.  Every term is non-negative, so any order of summing n terms is within
    (n - 1) 2^-53 relative of the exact sum and two orders within (n - 1) 2^-52 of each other; a term (three differences, three
    products, two sums) and the final combination (a product, two sums, a quotient) carry a handful of roundings more."""
    return (entries + 16) * 2.0 ** -52
