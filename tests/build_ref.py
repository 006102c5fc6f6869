"""numpy restatement of every stage of the hierarchy build (csrc/bvh_build.hip), for tests/test_build_stages_cpu.py (which holds
these restatements to definitions other than themselves, no GPU) and tests/test_build_stages_gpu.py (which holds what
fovpt_debug_build hands out of the production build to them).  Binary32 where the device is binary32: every product and sum is
rounded on its own (the library is built without contraction), fminf / fmaxf are exact.  No GPU, no library.

A binary tree is (left, right, root): arrays over the internal nodes, a child >= 0 being an internal node and < 0 the leaf at
sorted position ~child -- the build's own coding.  Two trees are compared by their canonical form (canonical), never by node ids:
which node of a Karras range or of a PLOC round carries which id is the kernels' business."""
import numpy as np

from refit_ref import F, INF, leaf_code, tri_boxes

LEAF_MAX = 4                      # FOVPT_LEAF_MAX
COST_LEAF = F(2.7)                # FOVPT_COST_LEAF: a leaf step of the collapse's programme, in node steps
COST_LEAF_STEP = F(1.4)           # FOVPT_COST_LEAF_STEP: a leaf step of the child order
PLOC_RADIUS = 16                  # FOVPT_PLOC_RADIUS
SPLIT_MAX = 8                     # FOVPT_SPLIT_MAX


# ---- boxes and bounds ----------------------------------------------------------------------------------------------------------
def centroid_bounds(lo, hi):
    """The exact min and max of 0.5f * (lo + hi) over the build primitives -> (6,) float32: min.xyz, max.xyz."""
    c = F(0.5) * (np.asarray(lo, F) + np.asarray(hi, F))
    return np.concatenate([c.min(axis=0), c.max(axis=0)]).astype(F)


def area32(lo, hi):
    """box_area / union_area: dx * dy + dy * dz + dz * dx, each product and sum rounded to binary32."""
    d = (np.asarray(hi, F) - np.asarray(lo, F)).astype(F)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return ((dx * dy).astype(F) + (dy * dz).astype(F)).astype(F) + (dz * dx).astype(F)


def area64(box):
    d = np.asarray(box, np.float64)[..., 3:6] - np.asarray(box, np.float64)[..., 0:3]
    return d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]


# ---- spatial splits ------------------------------------------------------------------------------------------------------------
def raw_bounds(p):
    p = np.asarray(p, F).reshape(-1, 3, 3)
    return np.fmin.reduce(p, axis=1), np.fmax.reduce(p, axis=1)


def split_count(p, s):
    """k = clamp(floor(longest extent / s), 1, FOVPT_SPLIT_MAX) per triangle, the division in binary32."""
    lo, hi = raw_bounds(p)
    ext = np.fmax(F(0), (hi - lo).astype(F).max(axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.floor((ext / F(s)).astype(F))
    return np.where(k >= SPLIT_MAX, SPLIT_MAX, np.where(k >= 1, k, 1)).astype(np.uint32)


def split_axis(p):
    """The first axis of the strictly longest extent (0 when every extent is 0)."""
    lo, hi = raw_bounds(p)
    return np.argmax((hi - lo).astype(F), axis=1)


def slab_planes(lo, hi, k):
    """The k + 1 planes of a box cut into k slabs along one axis: lo, lo + (hi - lo) * (j / k) in binary32, hi."""
    lo, hi = F(lo), F(hi)
    pl = [lo] + [F(lo + F(F(hi - lo) * F(F(j) / F(k)))) for j in range(1, k)] + [hi]
    return np.array(pl, F)


def clip_slab(tri, ax, c0, c1):
    """Sutherland-Hodgman in binary64: the triangle (3, 3) clipped to c0 <= x[ax] <= c1 -> polygon (m, 3), m = 0 when nothing is left."""
    poly = [np.asarray(v, np.float64) for v in np.asarray(tri, np.float64).reshape(3, 3)]
    for sign, c in ((1.0, float(c0)), (-1.0, float(c1))):
        out = []
        for i in range(len(poly)):
            a, b = poly[i], poly[(i + 1) % len(poly)]
            da, db = sign * (a[ax] - c), sign * (b[ax] - c)
            if da >= 0:
                out.append(a)
            if (da > 0 and db < 0) or (da < 0 and db > 0):
                t = da / (da - db)
                x = a + (b - a) * t
                x[ax] = c
                out.append(x)
        poly = out
        if not poly:
            break
    return np.array(poly, np.float64).reshape(-1, 3)


def split_references(p, count):
    """The references of every triangle in order: ref_prim, first (exclusive scan of count), and per reference (axis, c0, c1)."""
    count = np.asarray(count, np.int64)
    first = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.uint32)
    ref_prim = np.repeat(np.arange(len(count), dtype=np.uint32), count)
    lo, hi = raw_bounds(p)
    ax = split_axis(p)
    slabs = []
    for i, k in enumerate(count):
        pl = slab_planes(lo[i, ax[i]], hi[i, ax[i]], int(k))
        slabs += [(int(ax[i]), pl[j], pl[j + 1]) for j in range(int(k))]
    return ref_prim, first, slabs


def split_box32(tri, ax, c0, c1):
    """k_split_emit's box of one reference of a split triangle (k > 1) BEFORE the padding, in binary32: the vertices inside the
    slab and the points where the edges cross its two planes, clamped to the triangle's bounds."""
    p = np.asarray(tri, F).reshape(3, 3)
    lo, hi = p.min(axis=0), p.max(axis=0)
    blo, bhi = np.full(3, INF, F), np.full(3, -INF, F)
    c0, c1 = F(c0), F(c1)
    for e in range(3):
        u, v = p[e], p[(e + 1) % 3]
        if u[ax] >= c0 and u[ax] <= c1:
            blo, bhi = np.fmin(blo, u), np.fmax(bhi, u)
        for c in (c0, c1):
            if (u[ax] < c and v[ax] > c) or (u[ax] > c and v[ax] < c):
                t = F(F(c - u[ax]) / F(v[ax] - u[ax]))
                x = (u + ((v - u).astype(F) * t).astype(F)).astype(F)
                x[ax] = c
                blo, bhi = np.fmin(blo, x), np.fmax(bhi, x)
    if not blo[0] <= bhi[0]:
        blo, bhi = lo.copy(), hi.copy()
    return np.fmax(blo, lo), np.fmin(bhi, hi)


def tri_pads(p):
    """fovpt_tri_pad of every (whole) triangle: what tri_boxes adds on each side."""
    lo, hi = raw_bounds(p)
    plo, _ = tri_boxes(np.asarray(p, F).reshape(-1, 9))
    from refit_ref import tri_pad
    ext = np.fmax(F(0), (hi - lo).astype(F).max(axis=1))
    mag = np.fmax(F(0), np.fmax(np.abs(lo), np.abs(hi)).max(axis=1))
    return tri_pad(ext, mag)


# ---- Morton keys and the sort --------------------------------------------------------------------------------------------------
def quantise21(c, mn, mx):
    """k_morton's 21-bit cell of a centroid coordinate, in binary32: t = (c - mn) / (mx - mn) (0 when the extent is not
    positive), then min(max(t * 2^21, 0), 2^21 - 1) truncated."""
    c, mn, mx = np.asarray(c, F), F(mn), F(mx)
    ext = F(mx - mn)
    if ext > 0:
        t = ((c - mn).astype(F) / ext).astype(F)
    else:
        t = np.zeros_like(c)
    t = np.fmin(np.fmax((t * F(2097152.0)).astype(F), F(0)), F(2097151.0))
    return t.astype(np.uint32)


def interleave3(qx, qy, qz):
    """63-bit Morton key of three 21-bit numbers, bit by bit in Python integers: bit b of x, y, z lands at 3b + 2, 3b + 1, 3b."""
    key = 0
    for b in range(21):
        key |= ((int(qx) >> b) & 1) << (3 * b + 2)
        key |= ((int(qy) >> b) & 1) << (3 * b + 1)
        key |= ((int(qz) >> b) & 1) << (3 * b)
    return key


def morton_keys(lo, hi, cb):
    """Keys of the build primitives with padded boxes (lo, hi) under the centroid bounds cb -> (n,) uint64."""
    c = (F(0.5) * (np.asarray(lo, F) + np.asarray(hi, F))).astype(F)
    q = [quantise21(c[:, a], cb[a], cb[3 + a]) for a in range(3)]
    return np.array([interleave3(q[0][i], q[1][i], q[2][i]) for i in range(c.shape[0])], np.uint64)


def sort_keys(keys):
    """Stable by key (rocPRIM's radix sort is stable: equal keys keep primitive order) -> (keys_s, vals_s)."""
    order = np.argsort(np.asarray(keys, np.uint64), kind="stable")
    return np.asarray(keys, np.uint64)[order], order.astype(np.uint32)


# ---- trees in general ----------------------------------------------------------------------------------------------------------
def child_box(c, ibox, leaf_box):
    return leaf_box[~c] if c < 0 else ibox[c]


def post_order(left, right, root):
    """Internal nodes, children before parents."""
    order, stack = [], [int(root)]
    while stack:
        x = stack.pop()
        order.append(x)
        for c in (int(left[x]), int(right[x])):
            if c >= 0:
                stack.append(c)
    return order[::-1]


def union_boxes(left, right, root, leaf_box):
    """ibox (I, 6): the exact unions (fminf / fmaxf) of the children's boxes; leaf_box (n, 6) by sorted position."""
    ibox = np.zeros((len(left), 6), F)
    for x in post_order(left, right, root):
        a, b = child_box(int(left[x]), ibox, leaf_box), child_box(int(right[x]), ibox, leaf_box)
        ibox[x, 0:3], ibox[x, 3:6] = np.fmin(a[0:3], b[0:3]), np.fmax(a[3:6], b[3:6])
    return ibox


def shape_of(left, right, root, n):
    """size, first depth-first position and the depth-first position of every leaf, from the shape alone -> (size (I,),
    first (I,), leaf_pos (n,), leaves in depth-first order)."""
    size, first, leaf_pos = np.zeros(len(left), np.int64), np.zeros(len(left), np.int64), np.full(n, -1, np.int64)
    order, pos, stack = [], 0, [int(root)]
    seen = np.zeros(len(left), bool)
    while stack:
        c = stack.pop()
        if c < 0:
            assert leaf_pos[~c] < 0, "leaf %d twice" % ~c
            leaf_pos[~c] = pos
            order.append(~c)
            pos += 1
            continue
        assert not seen[c], "internal node %d twice" % c
        seen[c] = True
        first[c] = pos
        stack += [int(right[c]), int(left[c])]
    assert pos == n and (leaf_pos >= 0).all() and seen.all(), "not a binary tree over all %d leaves" % n
    for x in post_order(left, right, root):
        size[x] = sum(1 if c < 0 else size[c] for c in (int(left[x]), int(right[x])))
    return size, first, leaf_pos, np.array(order, np.int64)


def canonical(left, right, root, ibox, vals):
    """(primitive at each depth-first position, {(first position, size): the interval's box as bytes})."""
    size, first, _, order = shape_of(left, right, root, len(vals))
    boxes = {(int(first[x]), int(size[x])): np.asarray(ibox[x], F).tobytes() for x in range(len(left))}
    assert len(boxes) == len(left)
    return np.asarray(vals)[order].astype(np.int64), boxes


def tree_cost64(ibox):
    """Sum of the internal nodes' areas in binary64: what reinsertion lowers."""
    return float(area64(np.asarray(ibox, F)).sum())


# ---- Karras 2012 from its definition -------------------------------------------------------------------------------------------
def delta_fn(keys):
    """delta(i, j): the length of the common prefix of keys i and j, with the index as the tie-break for equal keys (64 + the
    common prefix of the 32-bit indices) and -1 outside the array."""
    ks = [int(k) for k in keys]
    n = len(ks)

    def delta(i, j):
        if j < 0 or j >= n:
            return -1
        if ks[i] == ks[j]:
            return 64 + (32 - (i ^ j).bit_length())
        return 64 - (ks[i] ^ ks[j]).bit_length()
    return delta


def karras(keys):
    """The binary radix tree over sorted keys by the definition, with linear scans (not k_hierarchy's doubling and binary
    searches): node i's range is the maximal run from i, towards the neighbour with the longer common prefix, of keys that
    share more with key i than the neighbour on the other side does; the split is the last position of the run whose prefix with
    i is longer than the whole range's.  -> (left, right, root = 0)."""
    n = len(keys)
    delta = delta_fn(keys)
    left, right = np.zeros(n - 1, np.int32), np.zeros(n - 1, np.int32)
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        dmin = delta(i, i - d)
        j = i
        while delta(i, j + d) > dmin:
            j += d
        dnode = delta(i, j)
        s = i
        while delta(i, s + d) > dnode:
            s += d
        gamma = s + min(d, 0)
        lo, hi = min(i, j), max(i, j)
        left[i] = ~gamma if lo == gamma else gamma
        right[i] = ~(gamma + 1) if hi == gamma + 1 else gamma + 1
    return left, right, 0


# ---- PLOC ----------------------------------------------------------------------------------------------------------------------
def union_area32(a, b):
    return area32(np.fmin(a[..., 0:3], b[..., 0:3]), np.fmax(a[..., 3:6], b[..., 3:6]))


def ploc_nearest(box, force):
    """k_ploc_nn over the clusters' boxes (m, 6): the partner of every cluster.  The first strict minimum of union_area in
    ascending j over the window of PLOC_RADIUS each side; itself when nothing is below +inf; i ^ 1 in a forced round."""
    m = box.shape[0]
    idx = np.arange(m)
    if force:
        j = idx ^ 1
        return np.where(j < m, j, idx)
    offs = np.array([o for o in range(-PLOC_RADIUS, PLOC_RADIUS + 1) if o != 0])
    cand = idx[:, None] + offs[None, :]
    ok = (cand >= 0) & (cand < m)
    cc = np.clip(cand, 0, m - 1)
    area = np.where(ok, union_area32(box[:, None, :], box[cc]), INF)
    best = np.argmin(area, axis=1)                        # (the first of equal minima)
    found = area[idx, best] < INF
    return np.where(found, cand[idx, best], idx)


def ploc(leaf_box, nearest=ploc_nearest):
    """PLOC over the sorted primitives' boxes (n, 6) -> dict(left, right, ibox, root, round_end, forced = the rounds that ran
    forced).  Mutual pairs merge at the lower index, survivors keep their order, and the pairs of a round take the next node
    ids in the order of their index, as on the device (where the ids come from the round's scan, not from an atomic)."""
    n = leaf_box.shape[0]
    left, right, ibox = np.zeros(n - 1, np.int32), np.zeros(n - 1, np.int32), np.zeros((n - 1, 6), F)
    node = [~i for i in range(n)]
    box = np.asarray(leaf_box, F).copy()
    made, force, round_end, forced = 0, 0, [], []
    while len(node) > 1:
        m = len(node)
        nn = nearest(box, force)
        forced.append(force)
        new_node, new_box = [], []
        for i in range(m):
            j = int(nn[i])
            if not (j != i and int(nn[j]) == i):
                new_node.append(node[i])
                new_box.append(box[i])
            elif i < j:
                u = np.concatenate([np.fmin(box[i, 0:3], box[j, 0:3]), np.fmax(box[i, 3:6], box[j, 3:6])])
                left[made], right[made], ibox[made] = node[i], node[j], u
                new_node.append(made)
                new_box.append(u)
                made += 1
        round_end.append(made)
        m2 = len(new_node)
        force = 1 if (m - m2) * 64 < m else 0
        node, box = new_node, np.array(new_box, F).reshape(-1, 6)
        assert len(round_end) <= 4096, "PLOC did not converge"
    return dict(left=left, right=right, ibox=ibox, root=n - 2, round_end=round_end, forced=forced)


# ---- the collapse's dynamic programme ------------------------------------------------------------------------------------------
def dp32(left, right, root, size, ibox, leaf_box):
    """dp_node over the whole tree in binary32, the comparisons as the kernel has them -> (I, 4) uint32: c1, c2, c3 (bits), dec."""
    out = np.zeros((len(left), 4), np.uint32)
    cost = np.zeros((len(left), 3), F)
    leaf_cost = (area32(leaf_box[:, 0:3], leaf_box[:, 3:6]) * COST_LEAF).astype(F)

    def child(c):
        return (leaf_cost[~c],) * 3 if c < 0 else tuple(cost[c])
    for x in post_order(left, right, root):
        l1, l2, l3 = child(int(left[x]))
        r1, r2, r3 = child(int(right[x]))
        s, dec = F(l1 + r3), 1
        if F(l2 + r2) < s:
            s, dec = F(l2 + r2), 2
        if F(l3 + r1) < s:
            s, dec = F(l3 + r1), 3
        area = area32(ibox[x, 0:3], ibox[x, 3:6])
        c1 = F(area + s)
        if size[x] <= LEAF_MAX and F(area * COST_LEAF) <= c1:
            c1, dec = F(area * COST_LEAF), dec | 4
        c2 = c1
        if F(l1 + r1) <= c2:
            c2, dec = F(l1 + r1), dec | 8
        c3, d3 = c2, 0
        if F(l1 + r2) <= c3:
            c3, d3 = F(l1 + r2), 1
        if F(l2 + r1) < c3:
            c3, d3 = F(l2 + r1), 2
        cost[x] = (c1, c2, c3)
        out[x, 3] = dec | (d3 << 4)
    out[:, 0:3] = cost.view(np.uint32)
    return out


def dp64(left, right, root, size, ibox, leaf_box):
    """The same recurrence in binary64 -> (I, 3): C(x, 1), C(x, 2), C(x, 3)."""
    cost = np.zeros((len(left), 3))
    leaf_cost = area64(leaf_box) * float(COST_LEAF)

    def child(c):
        return (leaf_cost[~c],) * 3 if c < 0 else tuple(cost[c])
    for x in post_order(left, right, root):
        l, r = child(int(left[x])), child(int(right[x]))
        area = float(area64(ibox[x]))
        c1 = area + min(l[0] + r[2], l[1] + r[1], l[2] + r[0])
        if size[x] <= LEAF_MAX:
            c1 = min(c1, area * float(COST_LEAF))
        c2 = min(c1, l[0] + r[0])
        c3 = min(c2, l[0] + r[1], l[1] + r[0])
        cost[x] = (c1, c2, c3)
    return cost


def brute_force_cost(left, right, root, size, ibox, leaf_box, slots=1):
    """The cheapest presentation of the tree in at most `slots` slots of a wide parent, by enumeration: every frontier of at
    most `slots` subtrees that covers the tree, every entry of it either a leaf (at most LEAF_MAX primitives: area x COST_LEAF)
    or a wide node (area x 1 + the cheapest frontier of at most four entries below it, itself excluded)."""
    memo_f, memo_e = {}, {}

    def frontiers(c, k):
        """every list of subtrees, at most k long, that covers subtree c"""
        if (c, k) not in memo_f:
            res = [[c]]
            if c >= 0:
                for a in range(1, k):
                    for fl in frontiers(int(left[c]), a):
                        for fr in frontiers(int(right[c]), k - a):
                            if len(fl) + len(fr) <= k and fl + fr not in res:
                                res.append(fl + fr)
            memo_f[(c, k)] = res
        return memo_f[(c, k)]

    def entry(c):
        if c not in memo_e:
            if c < 0:
                memo_e[c] = float(area64(leaf_box[~c])) * float(COST_LEAF)
            else:
                area = float(area64(ibox[c]))
                best = area + min(sum(entry(y) for y in f) for f in frontiers(c, 4) if f != [c])
                if size[c] <= LEAF_MAX:
                    best = min(best, area * float(COST_LEAF))
                memo_e[c] = best
        return memo_e[c]
    return min(sum(entry(y) for y in f) for f in frontiers(int(root), slots))


# ---- the collapse's emit -------------------------------------------------------------------------------------------------------
def wide_children(x, left, right, dec):
    """The entries of the wide node that binary node x becomes, in the order of k_collapse4's stack expansion: (subtree, slots)
    pairs are split as `dec` says until every pair fills one slot."""
    k = int(dec[x]) & 3
    stack = [(int(right[x]), 4 - k), (int(left[x]), k)]
    out = []
    while stack:
        y, sl = stack.pop()
        if y < 0 or sl == 1:
            out.append(y)
            continue
        d = int(dec[y])
        if sl == 3:
            d3 = (d >> 4) & 3
            if d3 == 1:
                stack += [(int(right[y]), 2), (int(left[y]), 1)]
                continue
            if d3 == 2:
                stack += [(int(right[y]), 1), (int(left[y]), 2)]
                continue
            sl = 2
        if d & 8:
            stack += [(int(right[y]), 1), (int(left[y]), 1)]
        else:
            out.append(y)
    assert 2 <= len(out) <= 4
    return out


def expected_entries(x, left, right, dec, size, node_first, leaf_pos, ibox, leaf_box):
    """The entries of x's wide node before the child order: per used slot (box (6,), leaf code or None for a child node, the
    binary node behind a child node or None)."""
    out = []
    for y in wide_children(x, left, right, dec):
        if y < 0:
            out.append((leaf_box[~y], leaf_code(int(leaf_pos[~y]), 1), None))
        elif int(dec[y]) & 4:
            out.append((ibox[y], leaf_code(int(node_first[y]), int(size[y])), None))
        else:
            out.append((ibox[y], None, y))
    return out


def wide_cost64(root, left, right, dec, size, ibox, leaf_box):
    """The cost, in the programme's units, of the wide tree the decisions give: every wide node its area, every leaf entry its
    area x COST_LEAF (binary64)."""
    total, stack = 0.0, [int(root)]
    while stack:
        x = stack.pop()
        total += float(area64(ibox[x]))
        for y in wide_children(x, left, right, dec):
            if y < 0:
                total += float(area64(leaf_box[~y])) * float(COST_LEAF)
            elif int(dec[y]) & 4:
                total += float(area64(ibox[y])) * float(COST_LEAF)
            else:
                stack.append(y)
    return total


# ---- the child order -----------------------------------------------------------------------------------------------------------
def order_children(nodes, tris, level_first):
    """k_order_children in binary32, deepest level first: nodes (N, 32) uint32 before the pass, tris (R, 12) uint32 -> the nodes
    after it."""
    nodes = np.array(nodes, np.uint32).reshape(-1, 32).copy()
    tf = np.asarray(tris, np.uint32).reshape(-1, 12).view(F)
    pc = np.zeros((nodes.shape[0], 2), F)
    one, two, half, zero = F(1), F(2), F(0.5), F(0)

    def sa_of(lo, hi):
        return F(two * area32(lo, hi))
    for L in range(len(level_first) - 2, -1, -1):
        for i in range(level_first[L], level_first[L + 1]):
            nd = nodes[i].reshape(4, 8).copy()
            nf, ni = nd.view(F), nd.view(np.int32)
            lo, hi = np.full(3, INF, F), np.full(3, -INF, F)
            P, C, sa, key = [zero] * 4, [one] * 4, [zero] * 4, [F(-1)] * 4
            for k in range(4):
                if not nf[k, 0] < INF:
                    continue
                lo, hi = np.fmin(lo, nf[k, 0:3]), np.fmax(hi, nf[k, 3:6])
                sa[k] = sa_of(nf[k, 0:3], nf[k, 3:6])
                code = int(ni[k, 6])
                if code < 0:
                    lcode = ~code & 0xffffffff
                    cnt, t0 = (lcode & 7) + 1, (lcode >> 3) // 3
                    area = zero
                    for T in tf[t0:t0 + cnt]:
                        e1, e2 = T[3:6], T[6:9]
                        cx = F(F(e1[1] * e2[2]) - F(e1[2] * e2[1]))
                        cy = F(F(e1[2] * e2[0]) - F(e1[0] * e2[2]))
                        cz = F(F(e1[0] * e2[1]) - F(e1[1] * e2[0]))
                        area = F(area + F(half * np.sqrt(F(F(F(cx * cx) + F(cy * cy)) + F(cz * cz)))))
                    P[k] = np.fmin(one, F(area / sa[k])) if sa[k] > 0 else one
                    C[k] = COST_LEAF_STEP
                else:
                    P[k], C[k] = pc[code]
                key[k] = F(P[k] / C[k])
            sa_node = sa_of(lo, hi)
            order = [0, 1, 2, 3]
            for a in range(1, 4):                          # insertion sort, descending, stable
                b = a
                while b > 0 and key[order[b]] > key[order[b - 1]]:
                    order[b], order[b - 1] = order[b - 1], order[b]
                    b -= 1
            passed, cost = one, one
            out = np.zeros((4, 8), np.uint32)
            for k in range(4):
                j = order[k]
                out[k] = nd[j]
                out[k, 7] = j
                if key[j] < 0:
                    continue
                h = np.fmin(one, F(sa[j] / sa_node)) if sa_node > 0 else one
                cost = F(cost + F(F(passed * h) * C[j]))
                passed = F(passed * F(one - F(h * P[j])))
            nodes[i] = out.reshape(32)
            pc[i] = (F(one - passed), cost)
    return nodes


# ---- a plain sequential reinsertion, binary64 ----------------------------------------------------------------------------------
def reinsert_sequential(left, right, root, leaf_box, max_moves=64):
    """One best positive-gain move at a time: take a node x (and its parent) out, put it back beside the node y that lowers the
    sum of the internal areas most, over all x and y; stop when no move gains.  Only shows that a tree has something to gain.
    Nodes here: internal 0 .. n-2, leaf at position l = n - 1 + l.  -> (cost before, cost after, moves made)."""
    n = leaf_box.shape[0]
    N = 2 * n - 1
    un = lambda c: (n - 1 + ~c) if c < 0 else c
    ch = np.full((N, 2), -1, np.int64)
    for x in range(n - 1):
        ch[x] = (un(int(left[x])), un(int(right[x])))
    root = int(root)
    lb = np.asarray(leaf_box, np.float64)

    def a64(b):
        d = b[..., 3:6] - b[..., 0:3]
        return d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]

    def union(a, b):
        return np.concatenate([np.minimum(a[..., 0:3], b[..., 0:3]), np.maximum(a[..., 3:6], b[..., 3:6])], axis=-1)

    def layout():
        parent = np.full(N, -1, np.int64)
        levels, cur = [], [root]
        tin, tout = np.zeros(N, np.int64), np.zeros(N, np.int64)
        while cur:
            levels.append(np.array(cur, np.int64))
            nxt = []
            for x in cur:
                if x < n - 1:
                    for c in ch[x]:
                        parent[c] = x
                        nxt.append(int(c))
            cur = nxt
        box = np.zeros((N, 6))
        box[n - 1:] = lb
        for lv in levels[::-1]:
            it = lv[lv < n - 1]
            box[it] = union(box[ch[it, 0]], box[ch[it, 1]])
        t, stack = 0, [(root, 0)]
        while stack:
            x, phase = stack.pop()
            if phase:
                tout[x] = t
                continue
            tin[x] = t
            t += 1
            stack.append((x, 1))
            if x < n - 1:
                stack += [(int(ch[x, 1]), 0), (int(ch[x, 0]), 0)]
        return parent, levels, box, tin, tout

    parent, levels, box, tin, tout = layout()
    cost0 = float(a64(box[:n - 1]).sum())
    moves = 0
    internal = np.arange(N) < n - 1
    while moves < max_moves:
        best = (1e-9 * cost0, -1, -1)
        for x in range(N):
            p = parent[x]
            if x == root or p == root:
                continue
            s = ch[p, 0] if ch[p, 1] == x else ch[p, 1]
            b2 = box.copy()
            b2[p] = box[s]                                   # p passes through: below q stands s alone
            removed, a, below = float(a64(box[p])), parent[p], p
            while a >= 0:
                other = ch[a, 0] if ch[a, 1] == below else ch[a, 1]
                b2[a] = union(b2[below], box[other])
                removed += float(a64(box[a]) - a64(b2[a]))
                below, a = a, parent[a]
            grow = a64(union(b2, box[x][None, :])) - a64(b2)          # what a node grows by when x comes to lie below it
            direct = grow + a64(b2)                                   # = area(y u x)
            contrib = np.where(internal, grow, 0.0)
            contrib[p] = 0.0
            inc = np.zeros(N)
            for lv in levels[1:]:
                inc[lv] = inc[parent[lv]] + contrib[parent[lv]]
            gain = removed - direct - inc
            gain[(tin >= tin[x]) & (tin < tout[x])] = -np.inf         # not into its own subtree
            gain[p] = -np.inf
            gain[s] = -np.inf                                         # (beside its sibling: where it is)
            y = int(np.argmax(gain))
            if gain[y] > best[0]:
                best = (float(gain[y]), x, y)
        if best[1] < 0:
            break
        _, x, y = best
        p = parent[x]
        q = parent[p]
        s = ch[p, 0] if ch[p, 1] == x else ch[p, 1]
        ch[q, 0 if ch[q, 0] == p else 1] = s
        parent[s] = q
        py = parent[y]
        ch[py, 0 if ch[py, 0] == y else 1] = p
        ch[p, 0 if ch[p, 1] == x else 1] = y
        parent, levels, box, tin, tout = layout()
        moves += 1
    return cost0, float(a64(box[:n - 1]).sum()), moves
