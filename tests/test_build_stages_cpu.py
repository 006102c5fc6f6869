"""The restatements of tests/build_ref.py held to definitions other than themselves, without a GPU: the Morton interleave against a
big-integer one, the Karras tree against a recursive top-down split, the vectorised PLOC round against a per-cluster loop, the
collapse's recurrence against an enumeration of every wide presentation, the slab clips against the triangle, and the scene of
the reinsertion test against a plain sequential reinsertion.  tests/test_build_stages_gpu.py then holds the production build to
the restatements stage by stage."""
import itertools

import numpy as np
import pytest

import build_ref as br
import build_stage_cases as bc
from refit_ref import F, tri_boxes


# ---- Morton --------------------------------------------------------------------------------------------------------------------
def _interleave_big(qx, qy, qz):
    """The digits of the three numbers written side by side: bit strings zipped, most significant first."""
    bits = ["{:021b}".format(int(q)) for q in (qx, qy, qz)]
    return int("".join(x + y + z for x, y, z in zip(*bits)), 2)


def test_morton_interleave_against_a_big_integer_one():
    rng = np.random.default_rng(1)
    q = rng.integers(0, 1 << 21, (500, 3))
    edge = [0, 1, 2, (1 << 20), (1 << 21) - 1, (1 << 21) - 2, 0x155555, 0x0aaaaa]
    q = np.concatenate([q, np.array(list(itertools.product(edge, repeat=3)))])
    for x, y, z in q:
        k = br.interleave3(x, y, z)
        assert k == _interleave_big(x, y, z) and k < (1 << 63)
    assert br.interleave3((1 << 21) - 1, 0, 0) == int("100" * 21, 2)             # x is the most significant of each triple
    assert br.interleave3(0, 0, (1 << 21) - 1) == int("001" * 21, 2)
    # the top bit of x outweighs everything below it, and a bit of y the same bit of z
    assert br.interleave3(1 << 20, 0, 0) > br.interleave3((1 << 20) - 1, (1 << 21) - 1, (1 << 21) - 1)
    assert br.interleave3(0, 4, 0) > br.interleave3(0, 3, 7) and br.interleave3(0, 4, 0) > br.interleave3(0, 0, 4)


def test_morton_quantisation_at_its_edges():
    mn, mx = F(-3.25), F(7.5)
    c = np.array([mn, mx, np.nextafter(mx, F(-np.inf)), np.nextafter(mn, F(np.inf)), F(2.125)], F)
    q = br.quantise21(c, mn, mx)
    assert q[0] == 0 and q[1] == (1 << 21) - 1 and q[2] in ((1 << 21) - 1, (1 << 21) - 2) and q[3] == 0
    exact = np.floor((np.float64(c[4]) - np.float64(mn)) / (np.float64(mx) - np.float64(mn)) * 2097152.0)
    assert abs(int(q[4]) - int(exact)) <= 1
    assert (br.quantise21(c, mn, mn) == 0).all()                                 # extent 0: every centroid in cell 0
    # random coordinates: within one cell of the binary64 quotient, never outside the grid
    rng = np.random.default_rng(2)
    c = rng.uniform(-3.25, 7.5, 4000).astype(F)
    q = br.quantise21(c, mn, mx).astype(np.int64)
    want = np.floor((c.astype(np.float64) - float(mn)) / (float(mx) - float(mn)) * 2097152.0)
    assert (np.abs(q - np.clip(want, 0, 2097151)) <= 1).all() and q.min() >= 0 and q.max() <= 2097151
    # whole keys: equal bounds give key 0, and keys order as x, then y, then z cells
    lo = np.zeros((3, 3), F)
    keys = br.morton_keys(lo, lo, np.zeros(6, F))
    assert (keys == 0).all()
    ks, vs = br.sort_keys(np.array([5, 3, 5, 3, 1], np.uint64))
    assert ks.tolist() == [1, 3, 3, 5, 5] and vs.tolist() == [4, 1, 3, 0, 2]    # stable


# ---- Karras --------------------------------------------------------------------------------------------------------------------
def _top_down(keys):
    """The radix tree by recursion: a range splits at the highest bit in which its (key, index) pairs differ -- the keys' bits
    first, then the index's for equal keys -- and its node is the end of the range next to the split... whose identity the
    canonical form does not need.  -> set of (first, size) intervals."""
    aug = [(int(k) << 32) | i for i, k in enumerate(keys)]
    out = set()

    def rec(a, b):                                          # [a, b]
        if a == b:
            return
        out.add((a, b - a + 1))
        top = (aug[a] ^ aug[b]).bit_length() - 1            # sorted: the highest differing bit of the ends is the range's
        m = a
        while not (aug[m + 1] >> top) & 1:
            m += 1
        rec(a, m)
        rec(m + 1, b)
    rec(0, len(keys) - 1)
    return out


@pytest.mark.parametrize("n", [2, 3, 5, 17, 64])
@pytest.mark.parametrize("kind", ["distinct", "equal", "runs"])
def test_karras_against_a_top_down_split(n, kind):
    rng = np.random.default_rng(10 * n + len(kind))
    if kind == "distinct":
        keys = np.sort(rng.choice(1 << 62, n, replace=False).astype(np.uint64))
    elif kind == "equal":
        keys = np.full(n, 0x1234567890abcde, np.uint64)
    else:
        keys = np.sort(rng.choice(rng.choice(1 << 62, max(2, n // 4), replace=False), n).astype(np.uint64))
    left, right, root = br.karras(keys)
    size, first, leaf_pos, order = br.shape_of(left, right, root, n)
    assert order.tolist() == list(range(n))                 # a radix tree keeps the sorted order
    assert {(int(f), int(s)) for f, s in zip(first, size)} == _top_down(keys)
    # delta over all pairs: every node's range shares a longer prefix inside than with either neighbour outside
    delta = br.delta_fn(keys)
    for f, s in zip(first, size):
        a, b = int(f), int(f + s - 1)
        inside = min(delta(i, j) for i in range(a, b + 1) for j in range(a, b + 1) if i != j)
        assert inside > max(delta(a, a - 1), delta(b, b + 1))


# ---- PLOC ----------------------------------------------------------------------------------------------------------------------
def _nearest_naive(box, force):
    m = box.shape[0]
    nn = np.zeros(m, np.int64)
    for i in range(m):
        if force:
            nn[i] = (i ^ 1) if (i ^ 1) < m else i
            continue
        best, bj = F(np.inf), i
        for j in range(max(0, i - br.PLOC_RADIUS), min(m - 1, i + br.PLOC_RADIUS) + 1):
            if j == i:
                continue
            d = np.fmax(box[i, 3:6], box[j, 3:6]) - np.fmin(box[i, 0:3], box[j, 0:3])
            a = F(F(F(d[0] * d[1]) + F(d[1] * d[2])) + F(d[2] * d[0]))
            if a < best:
                best, bj = a, j
        nn[i] = bj
    return nn


@pytest.mark.parametrize("kind", ["random", "equal", "lattice"])
def test_ploc_against_a_per_cluster_loop(kind):
    rng = np.random.default_rng(5)
    if kind == "random":
        lo = rng.uniform(-1, 1, (150, 3))
        box = np.concatenate([lo, lo + rng.uniform(0.01, 0.3, (150, 3))], axis=1).astype(F)
    elif kind == "equal":
        box = np.tile(np.array([[0, 0, 0, 1, 2, 3]], F), (130, 1))
    else:
        g = np.array(list(itertools.product(range(5), range(5), range(4))), F)
        box = np.concatenate([g, g + 1], axis=1).astype(F)
    a, b = br.ploc(box), br.ploc(box, nearest=_nearest_naive)
    assert a["round_end"] == b["round_end"] and a["forced"] == b["forced"]
    assert np.array_equal(a["left"], b["left"]) and np.array_equal(a["right"], b["right"]) and np.array_equal(a["ibox"], b["ibox"])
    n = box.shape[0]
    assert a["round_end"][-1] == n - 1
    assert np.array_equal(a["ibox"], br.union_boxes(a["left"], a["right"], a["root"], box))
    size, _, _, order = br.shape_of(a["left"], a["right"], a["root"], n)
    assert sorted(order.tolist()) == list(range(n)) and size[a["root"]] == n
    if kind == "equal":
        # among equal boxes everybody picks the first of its window: one pair per round, and the force rule takes over
        assert a["forced"][0] == 0 and a["round_end"][0] == 1 and a["forced"][1] == 1
        assert a["round_end"][1] == 1 + (n - 1) // 2
    else:
        assert not any(a["forced"])


# ---- the collapse's programme --------------------------------------------------------------------------------------------------
def _shapes(n, first=0):
    """Every binary tree shape over the leaves first .. first + n - 1 as nested tuples."""
    if n == 1:
        return [first]
    return [(l, r) for k in range(1, n) for l in _shapes(k, first) for r in _shapes(n - k, first + k)]


def _arrays(shape, n):
    """A nested-tuple tree -> (left, right, root) in the build's coding."""
    left, right = [], []

    def rec(t):
        if not isinstance(t, tuple):
            return ~t
        l, r = rec(t[0]), rec(t[1])
        left.append(l)
        right.append(r)
        return len(left) - 1
    root = rec(shape)
    return np.array(left, np.int32), np.array(right, np.int32), root


def _random_leaf_boxes(n, seed):
    rng = np.random.default_rng(seed)
    lo = rng.uniform(-1, 1, (n, 3))
    return np.concatenate([lo, lo + rng.uniform(0.0, 0.6, (n, 3)) * (rng.random((n, 3)) > 0.1)], axis=1).astype(F)


def _check_programme(left, right, root, leaf_box, with32=True):
    n = leaf_box.shape[0]
    size, first, leaf_pos, _ = br.shape_of(left, right, root, n)
    ibox = br.union_boxes(left, right, root, leaf_box)
    c64 = br.dp64(left, right, root, size, ibox, leaf_box)
    for slots in (1, 2, 3):
        want = br.brute_force_cost(left, right, root, size, ibox, leaf_box, slots)
        assert abs(c64[root, slots - 1] - want) <= 1e-12 * max(want, 1e-300), (slots, c64[root], want)
    if not with32:
        return None
    dp = br.dp32(left, right, root, size, ibox, leaf_box)
    c1 = float(dp[root, 0:1].view(F)[0])
    # the decisions, expanded, cost what the root's c1 says: binary32 sums of non-negative terms, one rounding per term
    dec = dp[:, 3].copy()
    dec[root] &= ~np.uint32(4)                              # (the root always becomes a wide node: k_collapse4 starts from it)
    got = br.wide_cost64(root, left, right, dec, size, ibox, leaf_box)
    if not int(dp[root, 3]) & 4:
        assert abs(got - c1) <= (4 * n + 8) * 2.0 ** -24 * max(c1, 1e-30), (got, c1)
    # binary32 against binary64: the same programme up to rounding
    assert np.allclose(dp[:, 0:3].view(F), c64, rtol=(4 * n + 8) * 2.0 ** -24, atol=1e-30)
    return dp


def test_collapse_programme_is_cost_optimal_on_every_shape():
    """Every tree shape of 2 to 10 leaves with random boxes over its leaves: the recurrence's C(root, 1..3) is the minimum
    over every presentation the enumeration finds (1e-12 relative: binary64 rounding only).  The binary32 restatement is held
    to both on every shape up to 7 leaves and on a sample of the larger ones."""
    checked = 0
    for n in range(2, 11):
        shapes = _shapes(n)
        leaf_box = _random_leaf_boxes(n, 100 + n)
        for k, shape in enumerate(shapes):
            left, right, root = _arrays(shape, n)
            _check_programme(left, right, root, leaf_box, with32=n <= 7 or k % 50 == 0)
            checked += 1
    assert checked == 1 + 2 + 5 + 14 + 42 + 132 + 429 + 1430 + 4862          # the Catalan numbers: every shape


def test_collapse_programme_on_degenerate_and_tied_boxes():
    """All boxes equal (every sum ties: `<` against `<=` decides) and all boxes points (every cost zero): still optimal, and
    ties dissolve the node -- a zero-cost tree must still get shallower."""
    for n in (5, 9):
        for leaf_box in (np.tile(np.array([[0, 0, 0, 1, 1, 1]], F), (n, 1)), np.zeros((n, 6), F)):
            for shape in _shapes(n)[::7]:
                left, right, root = _arrays(shape, n)
                dp = _check_programme(left, right, root, leaf_box)
                size, _, _, _ = br.shape_of(left, right, root, n)
                for x in range(len(left)):
                    if size[x] <= br.LEAF_MAX:
                        assert int(dp[x, 3]) & 4             # a leaf costs no more than anything below it here
                    kids = br.wide_children(x, left, right, dp[:, 3])
                    assert 2 <= len(kids) <= 4


# ---- splits --------------------------------------------------------------------------------------------------------------------
def test_split_slabs_clip_inside_the_box_and_cover_the_triangle():
    tri = bc.cards().reshape(-1, 9)
    lo, hi = br.raw_bounds(tri)
    ext = (hi - lo).max(axis=1)
    s = F(np.sort(ext)[-8] / 6.5)                           # the eight slivers are cut, nothing else is
    count = br.split_count(tri, s)
    assert (count > 1).sum() == 8 and count.max() <= br.SPLIT_MAX
    assert br.split_count(tri, F(1e-9)).max() == br.SPLIT_MAX and (br.split_count(tri, F(1e9)) == 1).all()
    ref_prim, first, slabs = br.split_references(tri, count)
    assert len(slabs) == count.sum() and np.array_equal(first, np.cumsum(count) - count)
    pads = br.tri_pads(tri)
    worst = 0.0
    for r, (ax, c0, c1) in enumerate(slabs):
        i = int(ref_prim[r])
        if count[i] == 1:
            continue
        poly = br.clip_slab(tri[i], ax, c0, c1)
        assert len(poly) >= 3
        assert (poly.min(axis=0) >= lo[i] - 1e-12).all() and (poly.max(axis=0) <= hi[i] + 1e-12).all()
        assert poly[:, ax].min() >= float(c0) and poly[:, ax].max() <= float(c1)
        blo, bhi = br.split_box32(tri[i], ax, c0, c1)
        over = max((poly.min(axis=0) - blo).max(), (bhi - poly.max(axis=0)).max()) / float(pads[i])
        under = max((blo - poly.min(axis=0)).max(), (poly.max(axis=0) - bhi).max()) / float(pads[i])
        worst = max(worst, over)
        assert under <= 1.0 and over <= 1.0                 # the binary32 box and the exact clip differ by less than one pad
    print("device box beyond the exact clip, in pads: %.3g" % worst)
    # the slabs of one triangle cover it: their areas add up to the triangle's, and consecutive slabs share their plane
    for i in np.flatnonzero(count > 1):
        t = tri[i].reshape(3, 3).astype(np.float64)
        total = 0.5 * np.linalg.norm(np.cross(t[1] - t[0], t[2] - t[0]))
        got = 0.0
        rs = range(int(first[i]), int(first[i]) + int(count[i]))
        for r in rs:
            poly = br.clip_slab(tri[i], *slabs[r])
            got += 0.5 * np.linalg.norm(sum(np.cross(poly[k] - poly[0], poly[k + 1] - poly[0]) for k in range(1, len(poly) - 1)))
        assert abs(got - total) <= 1e-9 * total
        assert slabs[rs[0]][1] == lo[i, slabs[rs[0]][0]] and slabs[rs[-1]][2] == hi[i, slabs[rs[0]][0]]
        assert all(slabs[r][2] == slabs[r + 1][1] for r in list(rs)[:-1])


def test_split_box_stays_within_two_pads_of_the_exact_clip():
    """Random references at scales 1e-3 to 1e3 and offsets up to 1e4: the restated device box (before the padding) exceeds the
    exact clip by less than one pad, so the padded box lies inside the clip grown by two."""
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(1500):
        scale, off = 10.0 ** rng.uniform(-3, 3), rng.uniform(-1, 1, 3) * 10.0 ** rng.uniform(0, 4)
        t = (rng.normal(0, 1, (3, 3)) * scale * np.array([1.0, rng.uniform(0.01, 1), rng.uniform(0.01, 1)]) + off).astype(F)
        lo, hi = br.raw_bounds(t.reshape(1, 9))
        ax = int(br.split_axis(t.reshape(1, 9))[0])
        k = int(rng.integers(2, br.SPLIT_MAX + 1))
        pl = br.slab_planes(lo[0, ax], hi[0, ax], k)
        pad = float(br.tri_pads(t.reshape(1, 9))[0])
        for j in range(k):
            poly = br.clip_slab(t, ax, pl[j], pl[j + 1])
            if len(poly) == 0:
                continue
            blo, bhi = br.split_box32(t, ax, pl[j], pl[j + 1])
            worst = max(worst, (poly.min(axis=0) - blo).max() / pad, (bhi - poly.max(axis=0)).max() / pad)
            assert (blo - poly.min(axis=0)).max() <= pad and (poly.max(axis=0) - bhi).max() <= pad
    print("device box beyond the exact clip, in pads: %.3g" % worst)
    assert worst <= 1.0


# ---- the child order -----------------------------------------------------------------------------------------------------------
def test_child_order_restatement_sorts_by_stopping_power():
    """One node of four leaf entries with one triangle each in equal boxes: the order is descending triangle area (P / C with
    equal C), pads keep the slots, an empty slot stays last, and the node's own P is 1 - prod(1 - h P)."""
    from refit_ref import leaf_code, records
    areas = [0.1, 0.4, 0.2]
    p = np.array([[0, 0, 0, 1, 0, 0, 0, 2 * a, 0] for a in areas], F)
    tris = records(p, np.arange(3), np.zeros(3))
    nodes = np.zeros((1, 32), np.uint32)
    nf, ni = nodes.view(F).reshape(1, 4, 8), nodes.view(np.int32).reshape(1, 4, 8)
    nf[0, :, 0:6] = np.inf
    for k in range(4):
        ni[0, k, 6], nodes.reshape(1, 4, 8)[0, k, 7] = leaf_code(0, 1), k
    for k in range(3):
        nf[0, k, 0:6] = (0, 0, 0, 1, 1, 1)
        ni[0, k, 6] = leaf_code(k, 1)
    out = br.order_children(nodes, tris, [0, 1]).reshape(4, 8)
    assert out[:, 7].tolist() == [1, 2, 0, 3]
    assert not out.view(F)[3, 0] < np.inf and (out.view(F)[0:3, 0] == 0).all()
    assert [int(c) for c in out.view(np.int32)[0:3, 6]] == [leaf_code(1, 1), leaf_code(2, 1), leaf_code(0, 1)]


# ---- the reinsertion scene -----------------------------------------------------------------------------------------------------
def test_cards_scene_has_something_to_gain_from_reinsertion():
    """The PLOC tree of the cards scene (slivers across a wall of small triangles) against a plain sequential reinsertion in
    binary64: the reference lowers the sum of the internal areas.  Measured: 3460.98 -> 3391.27 after 12 moves, 2.01 % lower."""
    tri = bc.cards().reshape(-1, 9)
    lo, hi = tri_boxes(tri)
    keys = br.morton_keys(lo, hi, br.centroid_bounds(lo, hi))
    _, vals = br.sort_keys(keys)
    leaf_box = np.concatenate([lo, hi], axis=1)[vals]
    t = br.ploc(leaf_box)
    before, after, moves = br.reinsert_sequential(t["left"], t["right"], t["root"], leaf_box, max_moves=12)
    print("cards: PLOC tree %.6g, after %d sequential moves %.6g (%.2f %% lower)" % (before, moves, after, 100 * (1 - after / before)))
    assert abs(before - br.tree_cost64(t["ibox"])) <= 1e-9 * before
    assert moves >= 1 and after < before
