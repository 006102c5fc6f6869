"""k_traverse ray by ray at its edges (csrc/traverse.hip): directions with exact zero components of either sign, origins
exactly on wall planes, hierarchies smaller than the root block kept in LDS, partly filled waves, several rounds per wave and
refilled occlusion pools, scaled and shifted scenes, spatial splits, refitted hierarchies.

Every case holds the library's closest hit (primitive, and t, u, v bit for bit) and occlusion flag against the oracle's brute
force over all triangles, and -- on the rays tests/trace_f64.py calls decided, in the configurations marked for it -- against
that binary64 statement of the contract directly, no oracle in between: primitive, occlusion flag, and t, u, v within the
tolerances recorded in tests/trace_cases.py.  tests/test_trace_edges_cpu.py shows without a GPU that the batches used here hit
and miss, are occluded and are not, and are decided often enough.  Everything goes through SampleRenderer.debug_trace: no test
reads a node or a triangle buffer."""
import numpy as np
import pytest

import trace_cases as tc
from fovpathtracing_optixcodelatest_amd import renderer
from trace_f64 import MISS, trace_f64

pytestmark = pytest.mark.gpu

_references = {}


def _reference(oracle, case, rays=None):
    """(origins, dirs, family per ray, the oracle's brute force, the binary64 result or None): computed once per configuration and
    shared by the builder variants."""
    key = case.name if rays is None else (case.name, len(rays[0]))
    if key not in _references:
        o, d, fam = rays if rays is not None else case.rays()
        want = oracle.OracleScene(tc.model_of(case.tri)).trace(o, d, brute=True)
        _references[key] = (o, d, fam, want, trace_f64(case.tri, o, d) if case.f64 else None)
    return _references[key]


def _compare(name, got, fam, want, f64, rows=slice(None)):
    """The library's (prim, tuv, occluded) for the rays `rows` of a batch against the references of those rays."""
    gp, gt, go = got
    wp, wt, wo = (x[rows] for x in want)
    fam = fam[rows]
    bad = np.flatnonzero(gp != wp)
    assert bad.size == 0, (name, "primitive", bad[:8], gp[bad[:8]], wp[bad[:8]])
    h = wp != MISS
    bad = np.flatnonzero((gt.view(np.uint32) != wt.view(np.uint32)).any(axis=1) & h)
    assert bad.size == 0, (name, "t, u, v bits", bad[:8], gt[bad[:8]], wt[bad[:8]])
    bad = np.flatnonzero(go != wo)
    assert bad.size == 0, (name, "occlusion", bad[:8], go[bad[:8]], wo[bad[:8]])
    if f64 is None:
        return
    fp, ft, fo, dec = (x[rows] for x in f64)
    bad = np.flatnonzero(dec & (gp != fp))
    assert bad.size == 0, (name, "primitive against binary64", bad[:8], gp[bad[:8]], fp[bad[:8]])
    bad = np.flatnonzero(dec & (go != fo))
    assert bad.size == 0, (name, "occlusion against binary64", bad[:8], go[bad[:8]], fo[bad[:8]])
    for k, f in enumerate(tc.FAMILIES):
        m = dec & (fp != MISS) & (fam == k)
        if m.any():
            t_rel = np.abs(gt[m, 0] - ft[m, 0]) / ft[m, 0]
            uv_abs = np.abs(gt[m, 1:] - ft[m, 1:])
            assert t_rel.max() <= tc.TOL_T_REL[f], (name, f, "t against binary64", t_rel.max())
            assert uv_abs.max() <= tc.TOL_UV_ABS[f], (name, f, "u, v against binary64", uv_abs.max())


def _trace_and_compare(oracle, r, case, rays=None):
    o, d, fam, want, f64 = _reference(oracle, case, rays)
    _compare(case.name, r.debug_trace(o, d), fam, want, f64)


@pytest.mark.parametrize("kind", ["soup", "lattice"])
@pytest.mark.parametrize("builder", sorted(tc.BUILDERS))
def test_tiny_hierarchies(oracle, monkeypatch, builder, kind):
    """1 to 160 triangles under every builder variant: a root with one leaf child, fewer nodes than the FOVPT_TOPN = 5 the kernel
    keeps in LDS, exactly as many or a few more, and more than 20; leaves of 1, 2, 3 and 4 triangles."""
    for k, v in tc.BUILDERS[builder].items():
        monkeypatch.setenv(k, v)
    nodes = {}
    for case in tc.tiny_cases(kind):
        r = renderer.SampleRenderer(tc.model_of(case.tri))
        nodes[case.name] = int(r.stats().num_bvh_nodes)
        try:
            _trace_and_compare(oracle, r, case)
        finally:
            r.close()
    print("num_bvh_nodes", builder, nodes)
    counts = list(nodes.values())
    assert min(counts) < 5, nodes                      # below FOVPT_TOPN: the kernel must not read s_top
    assert any(5 <= c <= 8 for c in counts), nodes     # at the boundary and just above it
    assert max(counts) > 20, nodes


def test_partial_waves(oracle):
    """Batches of 1 to 257 rays: waves whose 16 quads are only partly live vote and rank like full ones.  The first n rays of a
    batch give what they give inside the whole batch, and what the oracle gives."""
    for case in tc.exact_cases():
        o, d, fam, want, f64 = _reference(oracle, case)
        order = np.random.default_rng(7).permutation(len(o))            # (every family among the first few rays)
        o, d, fam = o[order], d[order], fam[order]
        want = tuple(x[order] for x in want)
        f64 = tuple(x[order] for x in f64) if f64 is not None else None
        r = renderer.SampleRenderer(tc.model_of(case.tri))
        try:
            full = r.debug_trace(o, d)
            _compare(case.name, full, fam, want, f64)
            for n in tc.PARTIAL_COUNTS:
                gp, gt, go = r.debug_trace(o[:n], d[:n])
                h = gp != MISS
                assert np.array_equal(gp, full[0][:n]) and np.array_equal(go, full[2][:n]), (case.name, n)
                assert np.array_equal(gt[h].view(np.uint32), full[1][:n][h].view(np.uint32)), (case.name, n)
                _compare("%s[:%d]" % (case.name, n), (gp, gt, go), fam, want, f64, slice(0, n))
        finally:
            r.close()


def test_exact_rays(oracle):
    """Axis-parallel directions with +0.0 and -0.0 in the other two components (safe_rcp turns them into +-1e20), origins on
    vertices, edges, diagonals and wall planes, rays inside a wall's plane, rays aimed at vertices and edges, rays that start on
    and just in front of a surface -- on the lattice and on the Cornell box, whose walls are axis-aligned too."""
    for case in tc.exact_cases():
        r = renderer.SampleRenderer(tc.model_of(case.tri))
        try:
            _trace_and_compare(oracle, r, case)
        finally:
            r.close()


def test_scaled_and_shifted_scenes(oracle):
    """All families on the lattice and a soup scaled by 1e3, 1e5 and 0.01 and moved to (1000, -2000, 500) and to 1e5: the box
    padding (1e-4 ext + 1e-5 mag) and the relative slack of the slab test at ray level."""
    for case in tc.magnitude_cases():
        r = renderer.SampleRenderer(tc.model_of(case.tri))
        try:
            _trace_and_compare(oracle, r, case)
        finally:
            r.close()


def test_rounds_and_refills(oracle, monkeypatch):
    """One unit per CU (FOVPT_GRID = FOVPT_GRID_SHADOW = 1): every closest-hit wave takes four full rounds and a partial one --
    a quad's LDS stack serves one ray after another -- and every occlusion wave's pool holds more than 60 rays, so it refills."""
    import torch
    monkeypatch.setenv("FOVPT_GRID", "1")
    monkeypatch.setenv("FOVPT_GRID_SHADOW", "1")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = (cus + 7) // 8 * 8 * 4
    n = 4 * 16 * waves + 37
    assert n > 16 * waves
    case = tc.rounds_case()
    o, d, fam = tc.rounds_rays(case, n)
    r = renderer.SampleRenderer(tc.model_of(case.tri))
    try:
        got = r.debug_trace(o, d)
    finally:
        r.close()
    want = oracle.OracleScene(tc.model_of(case.tri)).trace(o, d, brute=True)
    _compare(case.name, got, fam, want, None)
    # binary64 on every 8th ray (the loop over 300 triangles in numpy would take longer than everything else here)
    sub = slice(0, n, 8)
    _compare(case.name, tuple(x[sub] for x in got), fam[sub], tuple(x[sub] for x in want), trace_f64(case.tri, o[sub], d[sub]))


@pytest.mark.parametrize("rebuild", [False, True], ids=["refit", "rebuild"])
def test_after_update_vertices(oracle, rebuild):
    """The same ray checks after fovpt_update_vertices moved the mesh, against an oracle scene of the moved mesh: the refitted
    hierarchy (and the rebuilt one) of 1, 5, 17 and 65 triangles."""
    for case in tc.refit_cases():
        n = len(case.tri)
        r = renderer.SampleRenderer(tc.model_of(tc.soup(n, n)))
        try:
            r.update_vertices({0: case.tri.reshape(-1, 3)}, rebuild=rebuild)
            _trace_and_compare(oracle, r, case)
        finally:
            r.close()
