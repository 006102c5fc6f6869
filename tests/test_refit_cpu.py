"""CPU tests of tests/refit_ref.py, the restatement the GPU refit of fovpt_update_vertices is checked against, on hand-built wide
trees; and of the ABI mirror of fovpt_vertex_update."""

import numpy as np
import pytest

import header_layout
import refit_ref as rf
from fovpathtracing_optixcodelatest_amd import abi

F = np.float32
INF = F(np.inf)


def _scalar_box(p):
    """One triangle's padded box, one binary32 operation at a time (k_tri_bounds as written)."""
    lo, hi, ext, mag = [], [], F(0), F(0)
    for a in range(3):
        x0, x1, x2 = F(p[a]), F(p[3 + a]), F(p[6 + a])
        l, h = min(x0, min(x1, x2)), max(x0, max(x1, x2))
        lo.append(l), hi.append(h)
        ext = max(ext, F(h - l))
        mag = max(mag, max(F(abs(l)), F(abs(h))))
    pad = F(F(F(F(1e-4) * ext) + F(F(1e-5) * mag)) + F(1e-20))
    return np.array([F(l - pad) for l in lo], F), np.array([F(h + pad) for h in hi], F)


def _entry(lo, hi, code, rank):
    e = np.zeros(8, np.uint32)
    f = e.view(F)
    f[0:3], f[3:6] = lo, hi
    e[6] = np.uint32(np.int32(code).view(np.uint32))
    e[7] = rank
    return e


def _empty(rank):
    return _entry((INF, INF, INF), (INF, INF, INF), rf.leaf_code(0, 1), rank)


class Scene:
    """Random triangles over a shared vertex array, with per-primitive vertex indices and the records of the build."""

    def __init__(self, ntri, seed=0, scale=10.0):
        rng = np.random.default_rng(seed)
        self.vtx = (rng.standard_normal((ntri * 2 + 3, 3)) * scale).astype(F)
        self.vidx = rng.integers(0, self.vtx.shape[0], (ntri, 3))
        self.prim = np.arange(ntri, dtype=np.uint32)
        self.mesh = (self.prim % 3).astype(np.uint32)

    def p(self, vtx=None):
        v = self.vtx if vtx is None else vtx
        return v[self.vidx].reshape(-1, 9)

    def records(self, order, vtx=None):
        return rf.records(self.p(vtx)[order], self.prim[order], self.mesh[order])

    def box(self, recs, vtx=None):
        """The union of the padded boxes of the primitives recs, as the build forms it (fminf / fmaxf in order)."""
        boxes = [_scalar_box(q) for q in self.p(vtx)[recs]]
        lo, hi = boxes[0]
        for l, h in boxes[1:]:
            lo, hi = np.fmin(lo, l), np.fmax(hi, h)
        return lo, hi


def _two_level(sc, vtx=None):
    """Root: a node child (node 1, whose slots are leaves of 1, 2, 3 and 4 records), a leaf of 2 records, two empty slots.
    Records in leaf order: node 1's leaves (10), then the root's leaf (2)."""
    order = np.arange(12)
    recs = sc.records(order, vtx)
    n1 = np.zeros(32, np.uint32)
    first = 0
    for k, cnt in enumerate((1, 2, 3, 4)):
        n1[8 * k:8 * k + 8] = _entry(*sc.box(order[first:first + cnt], vtx), rf.leaf_code(first, cnt), k)
        first += cnt
    root = np.zeros(32, np.uint32)
    root[0:8] = _entry(*sc.box(order[0:10], vtx), 1, 0)
    root[8:16] = _entry(*sc.box(order[10:12], vtx), rf.leaf_code(10, 2), 1)
    root[16:24], root[24:32] = _empty(2), _empty(3)
    return np.stack([root, n1]), recs, [0, 1, 2]


def test_leaves_of_one_to_four_records_after_motion():
    sc = Scene(12, seed=1)
    nodes, tris, levels = _two_level(sc)
    moved = (sc.vtx * F(1.7) + F(3.25)).astype(F)
    got_n, got_t = rf.refit(nodes, tris, levels, sc.vidx, moved)
    want_n, want_t, _ = _two_level(sc, moved)
    assert np.array_equal(got_t, want_t)
    assert np.array_equal(got_n, want_n)
    assert not np.array_equal(got_n, nodes)


def test_empty_slots_are_left_alone():
    sc = Scene(12, seed=2)
    nodes, tris, levels = _two_level(sc)
    got_n, _ = rf.refit(nodes, tris, levels, sc.vidx, (sc.vtx * F(100)).astype(F))
    assert np.array_equal(got_n[0, 16:32], nodes[0, 16:32])              # both empty slots, codes and ranks included
    f = got_n.view(F).reshape(-1, 4, 8)
    assert np.isfinite(f[0, 0:2, 0:6]).all()                              # (a union over them would be +inf)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_tiny_scene_layout(n):
    """k_emit_tiny: one root whose first slot is a leaf of all n records, the other slots empty."""
    sc = Scene(n, seed=3 + n)
    order = np.arange(n)
    root = np.concatenate([_entry(*sc.box(order), rf.leaf_code(0, n), 0), _empty(1), _empty(2), _empty(3)])[None]
    recs = sc.records(order)
    moved = sc.vtx.copy()
    moved[:, 1] += F(5)
    got_n, got_t = rf.refit(root, recs, [0, 1], sc.vidx, moved)
    assert np.array_equal(got_t, sc.records(order, moved))
    want = np.concatenate([_entry(*sc.box(order, moved), rf.leaf_code(0, n), 0), _empty(1), _empty(2), _empty(3)])
    assert np.array_equal(got_n[0], want)


def test_identity_refit_reproduces_the_build():
    sc = Scene(12, seed=4)
    nodes, tris, levels = _two_level(sc)
    got_n, got_t = rf.refit(nodes, tris, levels, sc.vidx, sc.vtx)
    assert np.array_equal(got_n, nodes) and np.array_equal(got_t, tris)


@pytest.mark.parametrize("p", [
    [0.0] * 9,                                                            # ext = 0, mag = 0: pad 1e-20
    [3.5, -2.0, 7.0] * 3,                                                 # a point: ext = 0
    [1e6, 1e6, 1e6, 1e6 + 64, 1e6, 1e6, 1e6, 1e6 + 64, 1e6],              # large magnitude, small extent
    [-3e7, 0, 0, 3e7, 1, 0, 0, 2, 1e-3],                                  # large extent
    [1e-30, 0, 0, 0, 1e-30, 0, 0, 0, 1e-30],                              # tiny: pad below the coordinates' ulp
])
def test_padding_matches_the_scalar_expression(p):
    p = np.array(p, F)
    lo, hi = rf.tri_boxes(p[None])
    slo, shi = _scalar_box(p)
    assert np.array_equal(lo[0].view(np.uint32), slo.view(np.uint32)) and np.array_equal(hi[0].view(np.uint32), shi.view(np.uint32))
    v = p.reshape(3, 3)
    assert (lo[0] < v.min(axis=0)).all() and (hi[0] > v.max(axis=0)).all()    # strictly larger than the triangle's box
    assert rf.tri_pad(F(0), F(0)) == F(1e-20)
    assert rf.tri_pad(F(0), F(1e6)) == F(F(1e-5) * F(1e6)) + F(1e-20)


def test_conservative_check_and_levels():
    sc = Scene(12, seed=5)
    nodes, tris, levels = _two_level(sc)
    assert rf.levels_of(nodes) == levels
    moved = sc.vtx.copy()
    moved[sc.vidx[3]] += F(40)                                           # one triangle carried far away
    got_n, got_t = rf.refit(nodes, tris, levels, sc.vidx, moved)
    rf.check_conservative(got_n, got_t, levels)
    with pytest.raises(AssertionError):
        rf.check_conservative(nodes, got_t, levels)                      # the old boxes no longer hold the moved triangle
    assert rf.sah_cost(got_n, levels) >= 1.0


def test_abi_mirror_matches_the_header():
    (lay,), consts = header_layout.probe([("fovpt_vertex_update", ("mesh", "num_vertices", "vertex"))], ("FOVPT_UPDATE_DEVICE", "FOVPT_UPDATE_REBUILD"))
    got = lay + consts
    V = abi.VertexUpdate
    assert got == [C_size(V), V.mesh.offset, V.num_vertices.offset, V.vertex.offset, abi.UPDATE_DEVICE, abi.UPDATE_REBUILD]


def C_size(t):
    import ctypes
    return ctypes.sizeof(t)
