"""numpy float32 restatement of the refit of fovpt_update_vertices (csrc/refit.hip): the expected bytes of the hierarchy after
new vertex positions, from the bytes of the hierarchy before.

A hierarchy is what fovpt_debug_buffer hands out: "bvh_nodes", 128-byte wide nodes of four 32-byte child records
{lo.xyz, hi.xyz, code, rank} (code >= 0: a wide node, code < 0: a leaf, ~code = (first record in 16-byte units << 3) | (count - 1);
an empty slot has lo = hi = +inf), and "bvh_tris", 48-byte triangle records {v0, e1 = v1 - v0, e2 = v2 - v0, prim, mesh, pad}.
Here both are uint32 arrays, nodes (N, 32) and tris (R, 12).  levels: the wide tree's levels, level L being the nodes
[levels[L], levels[L + 1]) (children always lie on the next level).

The refit, deepest level first: a leaf entry rewrites its records from the vertices and becomes the union of their padded boxes;
a node entry becomes the union of its child node's non-empty entries; empty entries stay.  The padded box of a triangle is the
build's (bvh_build.hip k_tri_bounds): lo / hi per axis, pad = 1e-4 ext + 1e-5 mag + 1e-20 in binary32, ext the longest extent,
mag the largest coordinate magnitude.  Unions are fminf / fmaxf (np.fmin / np.fmax), which are exact."""
import numpy as np

F = np.float32
INF = F(np.inf)


def tri_pad(ext, mag):
    """fovpt_tri_pad: 1e-4f * ext + 1e-5f * mag + 1e-20f, each step rounded to binary32 (no fused multiply-add)."""
    ext, mag = np.asarray(ext, F), np.asarray(mag, F)
    return ((F(1e-4) * ext).astype(F) + (F(1e-5) * mag).astype(F)).astype(F) + F(1e-20)


def tri_boxes(p):
    """p (..., 9) float32 (v0, v1, v2) -> padded lo, hi (..., 3)."""
    p = np.asarray(p, F)
    v0, v1, v2 = p[..., 0:3], p[..., 3:6], p[..., 6:9]
    lo = np.fmin(v0, np.fmin(v1, v2))
    hi = np.fmax(v0, np.fmax(v1, v2))
    ext = np.fmax(F(0), (hi - lo).max(axis=-1))
    mag = np.fmax(F(0), np.fmax(np.abs(lo), np.abs(hi)).max(axis=-1))
    pad = tri_pad(ext, mag)[..., None]
    return (lo - pad).astype(F), (hi + pad).astype(F)


def records(p, prim, mesh):
    """The 48-byte triangle records of k_emit_tris_generic: p (R, 9) float32, prim / mesh (R,) -> (R, 12) uint32."""
    p = np.asarray(p, F)
    out = np.zeros((p.shape[0], 12), np.uint32)
    f = out.view(F)
    f[:, 0:3] = p[:, 0:3]
    f[:, 3:6] = p[:, 3:6] - p[:, 0:3]
    f[:, 6:9] = p[:, 6:9] - p[:, 0:3]
    out[:, 9], out[:, 10] = prim, mesh
    return out


def leaf_range(code):
    """A leaf entry's code -> (first record, count)."""
    lcode = ~int(code) & 0xffffffff
    return (lcode >> 3) // 3, (lcode & 7) + 1


def leaf_code(first, count):
    return ~(((first * 3) << 3) | (count - 1))


def refit(nodes, tris, levels, tri_vidx, vtx):
    """nodes (N, 32) uint32, tris (R, 12) uint32, levels, tri_vidx (T, 3) vertex indices per primitive, vtx (V, 3) float32 ->
    (nodes, tris) after the refit, new arrays."""
    nodes = np.array(nodes, np.uint32).reshape(-1, 32).copy()
    tris = np.array(tris, np.uint32).reshape(-1, 12).copy()
    tri_vidx = np.asarray(tri_vidx, np.int64).reshape(-1, 3)
    vtx = np.asarray(vtx, F).reshape(-1, 3)
    prim = tris[:, 9].astype(np.int64)
    p = vtx[tri_vidx[prim]].reshape(-1, 9)
    new = records(p, tris[:, 9], tris[:, 10])
    new[:, 11] = tris[:, 11]                                    # (the record's padding word is kept)
    tris = new
    rlo, rhi = tri_boxes(p)
    nf = nodes.view(F).reshape(-1, 4, 8)
    ni = nodes.view(np.int32).reshape(-1, 4, 8)
    for L in range(len(levels) - 2, -1, -1):
        for i in range(levels[L], levels[L + 1]):
            for k in range(4):
                if not nf[i, k, 0] < INF:
                    continue                                    # empty slot
                code = int(ni[i, k, 6])
                if code < 0:
                    t0, n = leaf_range(code)
                    lo = np.fmin.reduce(rlo[t0:t0 + n], axis=0)
                    hi = np.fmax.reduce(rhi[t0:t0 + n], axis=0)
                else:
                    ch = nf[code]
                    live = ch[:, 0] < INF
                    lo = np.fmin.reduce(np.where(live[:, None], ch[:, 0:3], INF), axis=0)
                    hi = np.fmax.reduce(np.where(live[:, None], ch[:, 3:6], -INF), axis=0)
                nf[i, k, 0:3], nf[i, k, 3:6] = lo, hi
    return nodes, tris


def check_conservative(nodes, tris, levels):
    """Every record's padded box lies inside its leaf entry, every child node's entries inside the parent's entry, every empty
    slot is +inf and every wide node but the root is some entry's child.  Raises AssertionError."""
    nf = np.asarray(nodes, np.uint32).reshape(-1, 32).view(F).reshape(-1, 4, 8)
    ni = np.asarray(nodes, np.uint32).reshape(-1, 32).view(np.int32).reshape(-1, 4, 8)
    tf = np.asarray(tris, np.uint32).reshape(-1, 12).view(F)
    v0 = tf[:, 0:3]
    p = np.concatenate([v0, (v0 + tf[:, 3:6]), (v0 + tf[:, 6:9])], axis=1)
    rlo = np.fmin(p[:, 0:3], np.fmin(p[:, 3:6], p[:, 6:9]))
    rhi = np.fmax(p[:, 0:3], np.fmax(p[:, 3:6], p[:, 6:9]))
    seen = np.zeros(nf.shape[0], bool)
    seen[0] = True
    for i in range(levels[-1]):
        for k in range(4):
            lo, hi = nf[i, k, 0:3], nf[i, k, 3:6]
            if not lo[0] < INF:
                assert (lo == INF).all() and (hi == INF).all(), "empty slot %d.%d is not +inf" % (i, k)
                continue
            assert (lo <= hi).all(), "entry %d.%d: lo > hi" % (i, k)
            code = int(ni[i, k, 6])
            if code < 0:
                t0, n = leaf_range(code)
                # (v0 + e1 may round: the records' corners are checked against the entry with the padding's slack)
                assert (rlo[t0:t0 + n] >= lo).all() and (rhi[t0:t0 + n] <= hi).all(), "records of leaf %d.%d outside it" % (i, k)
            else:
                seen[code] = True
                ch = nf[code]
                live = ch[:, 0] < INF
                assert live.any(), "node %d has no entries" % code
                assert (ch[live, 0:3] >= lo).all() and (ch[live, 3:6] <= hi).all(), "node %d outside entry %d.%d" % (code, i, k)
    assert seen[:levels[-1]].all(), "unreachable nodes"


def levels_of(nodes):
    """The levels of a wide tree from its bytes (breadth-first from the root, each level contiguous): [first node of level 0,
    of level 1, ..., the node count]."""
    ni = np.asarray(nodes, np.uint32).reshape(-1, 32).view(np.int32).reshape(-1, 4, 8)
    nf = ni.view(F)
    levels, lo, hi = [0], 0, 1
    while hi > lo:
        levels.append(hi)
        codes = ni[lo:hi, :, 6][(ni[lo:hi, :, 6] >= 0) & (nf[lo:hi, :, 0] < INF)]
        if codes.size == 0:
            break
        assert codes.min() == hi and codes.max() == hi + codes.size - 1, "the tree is not stored level by level"
        lo, hi = hi, hi + int(codes.size)
    return levels


def sah_cost(nodes, levels):
    """tools/bvhstat.py's SAH cost: the expected node steps of a random long ray plus 2.7 x its leaf steps (an entry is entered
    with probability area / root area), in node-step equivalents."""
    nf = np.asarray(nodes, np.uint32).reshape(-1, 32).view(F).reshape(-1, 4, 8)[:levels[-1], :, 0:6].astype(np.float64)
    code = np.asarray(nodes, np.uint32).reshape(-1, 32).view(np.int32).reshape(-1, 4, 8)[:levels[-1], :, 6]
    live = nf[:, :, 0] < np.inf
    d = np.where(live[..., None], nf[:, :, 3:6], 0.0) - np.where(live[..., None], nf[:, :, 0:3], 0.0)
    area = d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]
    lo = np.where(live[0, :, None], nf[0, :, 0:3], np.inf).min(axis=0)
    hi = np.where(live[0, :, None], nf[0, :, 3:6], -np.inf).max(axis=0)
    e = hi - lo
    root = e[0] * e[1] + e[1] * e[2] + e[2] * e[0]
    inner, leaf = live & (code >= 0), live & (code < 0)
    return float((root + area[inner].sum() + 2.7 * area[leaf].sum()) / root)
