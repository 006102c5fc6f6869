"""The ground the ray-level GPU tests (tests/test_trace_edges_gpu.py) stand on, checked without a GPU: for every scene and ray
family those tests use, the oracle's brute force equals the oracle's own BVH bit for bit and equals the binary64 statement of
the contract (tests/trace_f64.py) on every decided ray; the batches hit and miss, are occluded and are not, and are decided
often enough that the GPU tests cannot pass vacuously; and the tolerances the GPU tests use against binary64 are the oracle's
own measured deviations."""
import numpy as np

import trace_cases as tc
from trace_f64 import MISS, magnitude_ratio, trace_f64

_records = {}


def _record(oracle, case, o=None, d=None, fam=None):
    """Everything the tests below ask about one configuration, computed once."""
    key = case.name if o is None else (case.name, len(o))
    if key not in _records:
        if o is None:
            o, d, fam = case.rays()
        S = oracle.OracleScene(tc.model_of(case.tri))
        bp, bt, bo = S.trace(o, d, brute=True)
        hp, ht, ho = S.trace(o, d, brute=False)
        fp, ft, fo, dec = trace_f64(case.tri, o, d)
        _records[key] = dict(o=o, d=d, fam=fam, brute=(bp, bt, bo), bvh=(hp, ht, ho), f64=(fp, ft, fo), decided=dec,
                             ratio=magnitude_ratio(case.tri, o))
    return _records[key]


def _rounds(oracle):
    case = tc.rounds_case()
    o, d, fam = tc.rounds_rays(case, 4 * 16 * 1024 + 37)      # the batch of a device with 256 compute units
    return case, _record(oracle, case, o, d, fam)


def _all(oracle):
    return [(c, _record(oracle, c)) for c in tc.all_cases()] + [_rounds(oracle)]


def _of(rec, family):
    return rec["fam"] == tc.FAMILIES.index(family)


def test_oracle_brute_force_equals_its_bvh_bit_for_bit(oracle):
    for case, r in _all(oracle):
        (bp, bt, bo), (hp, ht, ho) = r["brute"], r["bvh"]
        assert np.array_equal(bp, hp), case.name
        h = bp != MISS
        assert np.array_equal(bt[h].view(np.uint32), ht[h].view(np.uint32)), case.name
        assert np.array_equal(bo, ho), case.name


def test_oracle_brute_force_equals_binary64_on_decided_rays(oracle):
    """Primitive and occlusion flag, ray by ray, in every configuration whose M / e allows it -- and the configurations marked
    for it are exactly those."""
    for case, r in _all(oracle):
        assert case.f64 == (r["ratio"] <= tc.MAX_RATIO_F64), (case.name, r["ratio"])
        if not case.f64:
            continue
        dec = r["decided"]
        (bp, bt, bo), (fp, ft, fo) = r["brute"], r["f64"]
        bad = dec & ((bp != fp) | (bo != fo))
        assert not bad.any(), (case.name, np.flatnonzero(bad)[:8], bp[bad][:8], fp[bad][:8], bo[bad][:8], fo[bad][:8])


def test_the_batches_cannot_pass_vacuously(oracle):
    for case, r in _all(oracle):
        bp, bt, bo = r["brute"]
        hit = bp != MISS
        assert 0 < bo.sum() < len(bo), case.name                                    # both outcomes of the occlusion ray
        for f in ("random", "aimed"):
            if f in case.families:
                share = hit[_of(r, f)].mean()
                assert 0.05 <= share <= 0.98, (case.name, f, share)
                assert 0 < bo[_of(r, f)].sum() < _of(r, f).sum(), (case.name, f)
        if not case.f64:
            continue
        dec = r["decided"]
        if "random" in case.families:
            assert dec[_of(r, "random")].mean() >= 0.9, (case.name, dec[_of(r, "random")].mean())
        if "axis" in case.families:
            assert dec[_of(r, "axis")].mean() >= 0.3, (case.name, dec[_of(r, "axis")].mean())
        assert (dec & hit).sum() > 0 and (dec & ~hit).sum() > 0, case.name
    # rays aimed at centroids, in a batch of their own (in the mixed batches they are a fifth of `aimed`)
    for case in tc.all_cases():
        if case.f64:
            o, d = tc.rays_aimed(case.tri, 300, case.seed, case.standoff, kind="centroid")
            dec = trace_f64(case.tri, o, d)[3]
            assert dec.mean() >= 0.9, (case.name, dec.mean())


def test_axis_rays_have_both_signs_of_zero_and_lie_on_the_walls():
    tri = tc.lattice(3)
    o, d, interior = tc.rays_axis(tri, 360, 1)
    zero = d == 0
    assert (zero.sum(1) == 2).all() and (np.abs(d).sum(1) == 1).all()
    assert (np.signbit(d) & zero).any(axis=1).sum() == len(d) // 2                  # the -0.0 copy
    assert np.array_equal(o[:len(o) // 4], o[len(o) // 4:len(o) // 2])              # ... of the same rays
    free = np.where(zero, o, 0.0)[~interior]
    assert (free == np.round(free * 2) / 2).all()                                   # on vertices and the middles of them
    oi, di = tc.rays_in_plane(tri, 100, 2)
    assert ((di == 0).sum(1) >= 1).all()                                            # exactly inside an axis-aligned plane


def measured_deviations(records):
    """The oracle's largest deviation from binary64 on decided hits, per family: t relative, u and v absolute."""
    t_rel = {f: 0.0 for f in tc.FAMILIES}
    uv_abs = {f: 0.0 for f in tc.FAMILIES}
    for case, r in records:
        if not case.f64:
            continue
        (bp, bt, bo), (fp, ft, fo) = r["brute"], r["f64"]
        ok = r["decided"] & (bp != MISS) & (bp == fp)
        for f in case.families:
            m = ok & _of(r, f)
            if m.any():
                t_rel[f] = max(t_rel[f], float((np.abs(bt[m, 0] - ft[m, 0]) / ft[m, 0]).max()))
                uv_abs[f] = max(uv_abs[f], float(np.abs(bt[m, 1:] - ft[m, 1:]).max()))
    return t_rel, uv_abs


def test_tolerances_are_the_measured_ones(oracle):
    """tc.TOL_T_REL / tc.TOL_UV_ABS hold 4 x the measured deviation, rounded up to two digits: the oracle itself is within
    them, and they are no wider than 4 x what is measured now (and that rounding)."""
    t_rel, uv_abs = measured_deviations(_all(oracle))
    print("measured: t", t_rel, "uv", uv_abs)
    for f in tc.FAMILIES:
        assert 0 < t_rel[f] <= tc.TOL_T_REL[f] <= 4.4 * t_rel[f], (f, t_rel[f])
        assert 0 < uv_abs[f] <= tc.TOL_UV_ABS[f] <= 4.4 * uv_abs[f], (f, uv_abs[f])


def test_binary64_contract_on_hand_made_rays():
    """tests/trace_f64.py itself: tmin is exclusive, equal t goes to the lower id, a back face occludes nothing."""
    tri = np.float32([[[0, 0, 1], [1, 0, 1], [0, 1, 1]], [[0, 0, 1], [2, 0, 1], [0, 2, 1]], [[0, 0, 2], [0, 1, 2], [1, 0, 2]]])
    o = np.float32([[0.25, 0.25, 0], [0.25, 0.25, 3], [0.25, 0.25, 1.5], [0.25, 0.25, 0.99], [5, 5, 0]])
    d = np.float32([[0, 0, 1], [0, 0, -1], [0, 0, 1], [0, 0, 1], [0, 0, 1]])
    prim, tuv, occ, dec = trace_f64(tri, o, d)
    assert prim.tolist() == [0, 2, 2, 2, MISS]
    assert tuv[0].tolist() == [1.0, 0.25, 0.25] and tuv[1, 0] == 1.0
    # from below triangles 0 and 1 show their back (e1 x e2 = +z, d = +z: det < 0) and triangle 2 its front
    assert occ.tolist() == [1, 1, 1, 1, 0]
    assert trace_f64(tri[:2], o[:1], d[:1])[2].tolist() == [0] and trace_f64(tri[:2], o[1:2], d[1:2])[2].tolist() == [1]
    assert dec.tolist() == [False, True, True, False, True]      # a tie; clear; clear; t = 0.01 - 1e-8 beside tmin; a clear miss
    prim, tuv, occ, dec = trace_f64(tri[[0, 0, 2]], o[:1], d[:1])     # an exact copy is no tie: the lower id has it
    assert prim.tolist() == [0] and dec.tolist() == [True]
