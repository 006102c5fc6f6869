"""CPU tests of tests/morph_ref.py, the restatement fovpt_update_morphed is checked against on the GPU: the arithmetic against a
scalar loop that rounds after every operation, hand-computed cases (the +-0 skip, the order of summation, dense and sparse,
the empty target), the overflow rules on either side of 2^127; and of the ABI mirrors of fovpt_morph_target, fovpt_mesh_morph
and fovpt_morph_pose."""
import ctypes

import numpy as np

import header_layout
import morph_ref as mr
import skin_ref as sk
from fovpathtracing_optixcodelatest_amd import abi

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _scalar(rest, targets, weights):
    """One vertex, one target and one operation at a time, every result rounded to binary32."""
    out = np.array(rest, F).reshape(-1, 3)
    lists = [mr.split(t, len(out)) for t in targets]
    with np.errstate(over="ignore", under="ignore"):
        for i in range(len(out)):
            p = [F(c) for c in out[i]]
            for t, (idx, d) in enumerate(lists):
                w = F(weights[t])
                hit = np.flatnonzero(idx == i)
                if w == 0 or not len(hit):
                    continue
                for a in range(3):
                    p[a] = F(p[a] + F(w * d[hit[0], a]))
            out[i] = p
    return out


REST = (np.random.default_rng(5).standard_normal((41, 3)) * 300).astype(F)


def test_apply_is_the_scalar_expression():
    rng = np.random.default_rng(21)
    for nt, dense in ((1, 1), (1, 0), (7, 2), (40, 3)):
        targets = mr.random_targets(rng, len(REST), nt, dense)
        for active in (0.0, 0.5, 1.0):
            w = mr.random_weights(rng, nt, active)
            assert mr.accepted(REST, targets, w)
            got = mr.apply(REST, targets, w)
            assert np.isfinite(got).all() and np.array_equal(_bits(got), _bits(_scalar(REST, targets, w)))
    # 1e-30 deltas under small weights: subnormal products
    tiny = [np.full((len(REST), 3), 1e-30, F)]
    assert np.array_equal(_bits(mr.apply(REST * F(1e-36), tiny, [1e-9])), _bits(_scalar(REST * F(1e-36), tiny, [1e-9])))


def test_a_zero_weight_skips_its_target_and_keeps_minus_zero():
    rest = np.array([[-0.0, 0.0, 1.0], [2.0, -0.0, -0.0]], F)
    targets = [np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0]], F), (np.array([1], np.uint32), np.array([[0.0, 0.0, 5.0]], F))]
    for w in ([0.0, 0.0], [-0.0, 0.0], [0.0, -0.0], [-0.0, -0.0]):
        assert np.array_equal(_bits(mr.apply(rest, targets, w)), _bits(rest))             # rest, bit for bit: the -0 stay -0
    # a weight that is not zero applies its target's zero deltas like any other entry: -0 + 1 * 0 = +0
    got = mr.apply(rest, targets, [1.0, 0.0])
    assert np.array_equal(_bits(got), _bits(np.array([[1.0, 2.0, 4.0], [2.0, 0.0, 0.0]], F)))
    assert not np.array_equal(_bits(got[1]), _bits(rest[1]))
    # ... and a vertex only the skipped target lists keeps its sign: target 1 alone lists vertex 1 alone (its -0 + 2 * 0 = +0)
    got = mr.apply(rest, targets, [0.0, 2.0])
    assert np.array_equal(_bits(got), _bits(np.array([[-0.0, 0.0, 1.0], [2.0, 0.0, 10.0]], F)))
    # an identity transform would not keep it: (1 * -0 + 0 * 0) + 0 * 1 + 0 = +0
    import transform_ref as tf
    assert not np.array_equal(_bits(tf.apply(rest, tf.IDENTITY)), _bits(rest))


def test_targets_are_summed_in_ascending_order():
    """1 + 2^24 = 2^24 in binary32 (a tie, to even), so ((1 + 2^24) - 2^24) + 1 = 1 while ((1 + 1) + 2^24) - 2^24 = 2."""
    rest = np.array([[1.0, 1.0, 1.0]], F)
    big, one = np.array([[2.0 ** 24, 0, 0]], F), np.array([[1.0, 0, 0]], F)
    asc = mr.apply(rest, [big, -big, one], [1, 1, 1])
    other = mr.apply(rest, [one, big, -big], [1, 1, 1])
    assert asc[0, 0] == 1.0 and other[0, 0] == 2.0
    # the weight multiplies the delta first, then the product is added: 3 * (1/3 rounded) is rounded before the sum
    third = F(1.0) / F(3.0)
    got = mr.apply(rest, [np.array([[third, 0, 0]], F)], [3.0])
    assert got[0, 0] == F(F(1.0) + F(F(3.0) * third))
    # skipping target 1 (weight -0) changes which sums are formed
    assert mr.apply(rest, [big, -big, one], [1, -0.0, 1])[0, 0] == F(2.0 ** 24)


def test_dense_is_sparse_with_every_index_and_an_empty_target_is_nothing():
    rng = np.random.default_rng(3)
    n = len(REST)
    dense = mr.random_targets(rng, n, 4, dense=4)
    sparse = [(np.arange(n, dtype=np.uint32), d) for d in dense]
    w = F([0.5, -1.25, 0.0, 2.0])
    assert np.array_equal(_bits(mr.apply(REST, dense, w)), _bits(mr.apply(REST, sparse, w)))
    empty = (np.zeros(0, np.uint32), np.zeros((0, 3), F))
    with_empty = [dense[0], empty, dense[1], empty, dense[2], dense[3]]
    assert np.array_equal(_bits(mr.apply(REST, with_empty, F([0.5, 7.0, -1.25, 0.0, 0.0, 2.0]))), _bits(mr.apply(REST, dense, w)))
    assert np.array_equal(_bits(mr.apply(REST, [empty], [3.0])), _bits(REST))
    assert list(mr.target_max(with_empty, n)[[1, 3]]) == [0.0, 0.0] and mr.target_max(dense, n)[0] == np.abs(dense[0]).max()
    assert mr.bound(REST, [empty], [1e38]) == np.abs(REST).max()                          # D = 0: any finite weight passes


def test_morph_then_skin_is_the_composition():
    rng = np.random.default_rng(8)
    targets, w = mr.random_targets(rng, len(REST), 5, 1), F([1.0, 0.0, -0.5, 0.25, 1.5])
    j, sw, nj = sk.random_skin(rng, len(REST), 4)
    pal = sk.random_pose(rng, REST, nj)
    assert mr.accepted(REST, targets, w, sw, pal)
    got = mr.apply_skinned(REST, targets, w, j, sw, pal)
    assert np.array_equal(_bits(got), _bits(sk.apply(_scalar(REST, targets, w), j, sw, pal)))
    assert np.array_equal(_bits(mr.apply_skinned(REST, targets, np.zeros(5, F), j, sw, pal)), _bits(sk.apply(REST, j, sw, pal)))


def test_overflow_bounds_on_either_side_of_two_to_the_127():
    rest = np.array([[2.0 ** 126, 0, 0], [0, -(2.0 ** 100), 1.0]], F)                     # A = 2^126
    t0 = np.array([[2.0 ** 100, 0, 0], [0, 0, -(2.0 ** 100)]], F)                        # D = 2^100
    t1 = (np.array([0], np.uint32), np.array([[0, 2.0 ** 90, 0]], F))                    # D = 2^90
    targets = [t0, t1]
    assert list(mr.target_max(targets, 2)) == [2.0 ** 100, 2.0 ** 90]
    w = F([2.0 ** 25, -(2.0 ** 35)])                                                      # 2^126 + 2^125 + 2^125 = 2^127: not above
    assert mr.bound(rest, targets, w) == 2.0 ** 127 and mr.accepted(rest, targets, w)
    assert np.isfinite(mr.apply(rest, targets, w)).all()
    for k in (0, 1):                                                                      # one ulp more on either weight
        w2 = w.copy()
        w2[k] = np.nextafter(w[k], F(np.inf) * np.sign(w[k]))
        assert mr.bound(rest, targets, w2) > 2.0 ** 127 and not mr.accepted(rest, targets, w2)
    assert mr.accepted(rest, targets, F([-(2.0 ** 25), 2.0 ** 35]))                       # the bound adds magnitudes
    assert mr.accepted(np.zeros((0, 3), F), [], [])                                       # nothing at all
    for bad in (np.nan, np.inf, -np.inf):
        assert not mr.accepted(rest, targets, F([bad, 0.0])) and not mr.accepted(rest, targets, F([0.0, bad]))
    # -- with a palette: skin_ref's two rules with B in A's place
    small = np.array([[2.0 ** -40, 0, 0]], F)
    tiny = [np.array([[2.0 ** -41, 0, 0]], F)]
    j, w4 = np.zeros((1, 4), np.uint16), np.ones((1, 4), F)                               # S = 4
    one = F([1.0])
    assert mr.bound(small, tiny, one) == 2.0 ** -40 + 2.0 ** -41
    # (1) the row rule alone would let this through (B < 1 makes the row's bound small); the entry rule refuses it, and the
    #     blended matrix does overflow
    pal = np.zeros((1, 3, 4), F)
    pal[0, 0, 0] = F(2.0 ** 127)
    assert mr.row_bound(small, tiny, one, w4, pal) < 2.0 ** 127 and mr.entry_bound(w4, pal) > 2.0 ** 127
    assert not mr.accepted(small, tiny, one, w4, pal)
    assert not np.isfinite(mr.apply_skinned(small, tiny, one, j, w4, pal)).all()
    # (2) the entry rule alone would let this through, and so would the row rule with A instead of B: the morph carries the
    #     vertex to 2^100, and the row's product overflows
    far = [np.array([[2.0 ** 100, 0, 0]], F)]
    pal = np.zeros((1, 3, 4), F)
    pal[0, 0, 0] = F(2.0 ** 26)
    assert mr.entry_bound(w4, pal) == 2.0 ** 28 and sk.accepted(small, w4, pal)
    assert mr.row_bound(small, far, one, w4, pal) > 2.0 ** 127 and not mr.accepted(small, far, one, w4, pal)
    assert not np.isfinite(mr.apply_skinned(small, far, one, j, w4, pal)).all()
    assert mr.accepted(small, far, F([0.0]), w4, pal) and mr.accepted(small, far, one, w4, pal * F(0.25))
    assert np.isfinite(mr.apply_skinned(small, far, one, j, w4, pal * F(0.25))).all()
    # exactly 2^127 is not above: S (m0 B) = 4 * 2^25 * 2^100 with B = 2^100 exactly
    exact = [np.array([[2.0 ** 100 - 2.0 ** -40, 0, 0]], F)]                              # (rounds to 2^100 in binary32 ...)
    assert exact[0][0, 0] == F(2.0 ** 100)
    zero = np.zeros((1, 3), F)
    pal[0, 0, 0] = F(2.0 ** 25)
    assert mr.row_bound(zero, exact, one, w4, pal) == 2.0 ** 127 and mr.accepted(zero, exact, one, w4, pal)
    pal[0, 0, 3] = F(2.0 ** 80)                                                           # S (2^125 + 2^80), exact in binary64
    assert not mr.accepted(zero, exact, one, w4, pal)
    for bad in (np.nan, np.inf, -np.inf):
        pal = np.tile(F([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]), (1, 1, 1))
        pal[0, 1, 3] = bad
        assert not mr.accepted(small, tiny, one, w4, pal)
    # within the bounds nothing overflows, whatever the signs and the weights
    rng = np.random.default_rng(9)
    n_accepted = 0
    for k in range(60):
        r = (rng.choice([-1.0, 1.0], (32, 3)) * 2.0 ** rng.uniform(100, 126, (32, 3))).astype(F)
        ts = [(rng.choice([-1.0, 1.0], (32, 3)) * 2.0 ** rng.uniform(60, 100, (32, 3))).astype(F) for _ in range(6)]
        ws = (rng.choice([-1.0, 1.0], 6) * 2.0 ** rng.uniform(10, 25.5, 6)).astype(F)
        if mr.accepted(r, ts, ws):
            n_accepted += 1
            assert np.isfinite(mr.apply(r, ts, ws)).all()
    assert 10 < n_accepted < 60


def test_procedural_targets_are_what_they_say():
    ts = mr.bumps(REST, 3, 5, 0.1)
    assert len(ts) == 8 and all(t.shape == REST.shape for t in ts[:3])
    for idx, d in ts[3:]:
        assert idx.dtype == np.uint32 and len(idx) == 4 and (np.diff(idx.astype(np.int64)) > 0).all() and d.shape == (4, 3)
    rng = np.random.default_rng(1)
    w = np.concatenate([mr.random_weights(rng, 64) for _ in range(4)])
    assert (w == 0).any() and np.signbit(w[w == 0]).any() and not np.signbit(w[w == 0]).all() and (w < 0).any() and (w > 1).any()


def test_abi_mirrors_match_the_header():
    (t, m, p), consts = header_layout.probe(
        [("fovpt_morph_target", ("count", "_reserved", "index", "delta")),
         ("fovpt_mesh_morph", ("mesh", "num_vertices", "num_targets", "_reserved", "targets")),
         ("fovpt_morph_pose", ("mesh", "num_targets", "weights", "num_joints", "_reserved", "matrices"))],
        ("sizeof(void*)", "FOVPT_MORPH_MAX_TARGETS"))
    got = t + m + p + consts
    T, M, P = abi.MorphTarget, abi.MeshMorph, abi.MorphPose
    assert got == [ctypes.sizeof(T), T.count.offset, T._reserved.offset, T.index.offset, T.delta.offset,
                   ctypes.sizeof(M), M.mesh.offset, M.num_vertices.offset, M.num_targets.offset, M._reserved.offset, M.targets.offset,
                   ctypes.sizeof(P), P.mesh.offset, P.num_targets.offset, P.weights.offset, P.num_joints.offset, P._reserved.offset,
                   P.matrices.offset, ctypes.sizeof(ctypes.c_void_p), abi.MORPH_MAX_TARGETS]
    assert (got[0], got[5], got[11], got[-1]) == (24, 24, 32, 256) and mr.MAX_TARGETS == 256
