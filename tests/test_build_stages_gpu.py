"""Every stage of the production hierarchy build (csrc/bvh_build.hip) against its restatement (tests/build_ref.py), on what
fovpt_debug_build hands out of fovpt_build_lbvh itself: splits, boxes, centroid bounds, Morton keys, the sort, the Karras tree,
PLOC, reinsertion, the collapse's dynamic programme under its three drivers, the emitted wide tree, the child order and the
triangle records.  No ray is traced here: results never depend on the tree, so nothing that traces can see these stages.

Exact pins are bit for bit.  Wide-node slots come from an atomic and node ids are the kernels' business, so trees are compared
by canonical form (binary trees) or walked from the root beside the restatement (the wide tree), never index by index.
Reinsertion's concurrent moves are held to invariants (still a tree over the same leaves, exact boxes, consistent sizes and
positions), and to a lower cost on the one scene built for it."""
import ctypes as C

import numpy as np
import pytest

import build_ref as br
import build_stage_cases as bc
import refit_ref as rf
import trace_cases as tc
from fovpathtracing_optixcodelatest_amd import renderer, scenes
from refit_ref import F, INF

pytestmark = pytest.mark.gpu

REINSERT_DEFAULT = 12             # FOVPT_REINSERT_DEFAULT
# (PLOC, split budget, reinsertion rounds, child order)
CONFIGS = {
    "ploc": (True, 0.0, 0, True),
    "ploc_reinsert_noorder": (True, 0.0, REINSERT_DEFAULT, False),
    "lbvh": (False, 0.0, 0, True),
    "ploc_split_reinsert": (True, 1.0, REINSERT_DEFAULT, True),
    "lbvh_split_noorder": (False, 1.0, 0, False),
    # a budget too small for one extra reference of the lattice's 216 triangles (< 1 / 216): the split stage counts, makes no
    # reference, and the build goes on over the triangles' own boxes
    "ploc_split_none": (True, 1.0 / 256.0, 0, True),
}
SCENES = {
    "soup1": lambda: tc.soup(1, 1), "soup4": lambda: tc.soup(4, 2), "soup5": lambda: tc.soup(5, 3), "soup17": lambda: tc.soup(17, 4),
    "soup64": lambda: tc.soup(64, 5), "soup65": lambda: tc.soup(65, 6), "soup256": lambda: tc.soup(256, 7), "soup257": lambda: tc.soup(257, 8),
    "soup300": lambda: tc.soup(300, 9, scale=3.0, offset=(10.0, -4.0, 2.0)), "soup2000": lambda: tc.soup(2000, 10),
    "duplicates": bc.duplicates, "lattice": lambda: tc.lattice(6), "cards": bc.cards,
}
_three = ("ploc", "ploc_reinsert_noorder", "lbvh")
CASES = [("soup1", "ploc"), ("soup4", "ploc"), ("soup4", "ploc_split_reinsert"), ("soup4", "lbvh")]
CASES += [(s, c) for s in ("soup5", "soup17", "soup64", "soup65", "soup256", "soup257", "soup300", "soup2000", "duplicates", "lattice", "cards") for c in _three]
CASES += [(s, "ploc_split_reinsert") for s in ("soup5", "soup17", "soup65", "soup300", "soup2000", "cards")]
CASES += [(s, "lbvh_split_noorder") for s in ("soup300", "cards")]
CASES += [("lattice", "ploc_split_none")]

_scene_cache, _ref_cache = {}, {}


def scene(name):
    if name not in _scene_cache:
        _scene_cache[name] = np.ascontiguousarray(SCENES[name](), np.float32)
    return _scene_cache[name]


@pytest.fixture(scope="module")
def hook():
    """A context to call the hook on: it needs no scene of its own and must not touch this one."""
    r = renderer.SampleRenderer(scenes.cornell_box())
    before = hierarchy(r)
    yield r
    after = hierarchy(r)
    assert all(np.array_equal(a, b) for a, b in zip(before, after)), "fovpt_debug_build changed the context's own hierarchy"
    r.close()


def hierarchy(r):
    out = []
    for name, width in ((b"bvh_nodes", 32), (b"bvh_tris", 12)):
        p, n = C.c_void_p(), C.c_size_t()
        r._check(r._L.fovpt_debug_buffer(r._ctx, name, C.byref(p), C.byref(n)))
        out.append(r.download(p.value, np.empty(n.value // 4, np.uint32)).reshape(-1, width))
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def wide_canonical(nodes, num_nodes):
    """The wide tree without its node numbers: per node its four entries in slot order as (box bytes, rank, leaf code or the
    child node's own form)."""
    nodes = np.asarray(nodes, np.uint32).reshape(-1, 4, 8)
    ni = nodes.view(np.int32)

    def rec(w, depth):
        assert depth < 80
        out = []
        for k in range(4):
            live = nodes[w, k, 0:1].view(F)[0] < INF
            code = int(ni[w, k, 6])
            sub = rec(code, depth + 1) if (live and code >= 0) else code
            out.append((nodes[w, k, 0:6].tobytes(), int(nodes[w, k, 7]), sub))
        return tuple(out)
    assert num_nodes >= 1
    return rec(0, 0)


# ---- the checks, stage by stage -------------------------------------------------------------------------------------------------
def check_splits(p, budget, T):
    """-> (per-reference triangle, True where a reference is one of several)."""
    n = p.shape[0]
    if not (budget > 0 and n > br.LEAF_MAX):
        assert not T["have_count"] and not T["have_splits"] and T["num_refs"] == n
        return np.arange(n), np.zeros(n, bool)
    assert T["have_count"] and T["s_cut"] > 0
    count = br.split_count(p, T["s_cut"])
    assert np.array_equal(T["split_count"], count)
    total = int(count.sum())
    assert total <= (1.0 + budget) * n
    if total == n:
        assert not T["have_splits"] and T["num_refs"] == n and (T["split_count"] == 1).all()
        return np.arange(n), np.zeros(n, bool)
    assert T["have_splits"] and T["num_refs"] == total
    ref_prim, first, slabs = br.split_references(p, count)
    assert np.array_equal(T["split_first"], first) and np.array_equal(T["ref_prim"], ref_prim)
    wlo, whi = rf.tri_boxes(p)
    pads = br.tri_pads(p).astype(np.float64)
    blo, bhi = T["boxes"][:, 0:3], T["boxes"][:, 3:6]
    multi = count[ref_prim] > 1
    # a triangle that is not cut keeps its whole box
    assert same_bits(blo[~multi], wlo[ref_prim[~multi]]) and same_bits(bhi[~multi], whi[ref_prim[~multi]])
    whole_passes = 0
    for r in np.flatnonzero(multi):
        i = int(ref_prim[r])
        poly = br.clip_slab(p[i], *slabs[r])
        assert len(poly) >= 3, ("empty slab", r)
        clo, chi = poly.min(axis=0), poly.max(axis=0)
        assert (blo[r] <= clo).all() and (bhi[r] >= chi).all(), ("reference does not contain its clip", r)
        assert (blo[r] >= wlo[i]).all() and (bhi[r] <= whi[i]).all(), ("reference outside the triangle's box", r)
        assert (blo[r] >= clo - 2 * pads[i]).all() and (bhi[r] <= chi + 2 * pads[i]).all(), ("reference is not the clip's box", r)
        whole_passes += bool((wlo[i] >= clo - 2 * pads[i]).all() and (whi[i] <= chi + 2 * pads[i]).all())
    assert whole_passes == 0, "the whole box would pass the tightness check: it checks nothing"
    return ref_prim.astype(np.int64), multi


def check_tiny(p, T, mesh):
    n = p.shape[0]
    assert n <= br.LEAF_MAX and T["num_refs"] == n and T["num_nodes"] == 1 and T["max_depth"] == 1 and T["level_first"] == [0, 1]
    assert T["keys_s"] is None and T["left0"] is None and T["dp"] is None and not T["reinserted"]
    assert np.array_equal(T["vals_s"], np.arange(n)) and np.array_equal(T["leaf_pos"], np.arange(n))
    want = np.zeros((4, 8), np.uint32)
    want.view(F)[:, 0:6] = INF
    want.view(np.int32)[:, 6] = rf.leaf_code(0, 1)
    want[:, 7] = np.arange(4)
    want.view(F)[0, 0:3], want.view(F)[0, 3:6] = T["boxes"][:, 0:3].min(axis=0), T["boxes"][:, 3:6].max(axis=0)
    want.view(np.int32)[0, 6] = rf.leaf_code(0, n)
    assert same_bits(T["nodes_pre"], want.reshape(1, 32)) and same_bits(T["nodes"], want.reshape(1, 32))      # (a tiny build is not reordered)
    assert same_bits(T["tris"], rf.records(p, np.arange(n), mesh))


def reference_stages(key, boxes, ploc):
    """Keys, sort and the PLOC / Karras tree over these boxes: computed once per (scene, boxes) and shared by the configurations."""
    ck = (key, boxes.tobytes()[:64], boxes.shape[0])
    if ck not in _ref_cache:
        cb = br.centroid_bounds(boxes[:, 0:3], boxes[:, 3:6])
        keys = br.morton_keys(boxes[:, 0:3], boxes[:, 3:6], cb)
        ks, vs = br.sort_keys(keys)
        _ref_cache[ck] = dict(cb=cb, keys=keys, ks=ks, vs=vs, leaf_box=boxes[vs])
    R = _ref_cache[ck]
    name = "ploc" if ploc else "karras"
    if name not in R:
        if ploc:
            R[name] = br.ploc(R["leaf_box"])
        else:
            left, right, root = br.karras(R["ks"])
            R[name] = dict(left=left, right=right, root=root, ibox=br.union_boxes(left, right, root, R["leaf_box"]))
        t = R[name]
        t["canonical"] = br.canonical(t["left"], t["right"], t["root"], t["ibox"], R["vs"])
    return R, R[name]


def check_wide_tree(T, root, dec, leaf_box):
    """Walk the wide tree as emitted (before the child order) from node 0 beside the binary tree the collapse saw."""
    N = T["num_nodes"]
    nodes = T["nodes_pre"].reshape(-1, 4, 8)
    nf, ni = nodes.view(F), nodes.view(np.int32)
    referenced, depth_of = np.zeros(N, np.int64), np.zeros(N, np.int64)
    depth_of[0] = 1
    stack, visited, leaves = [(0, int(root))], 0, []
    while stack:
        w, x = stack.pop()
        visited += 1
        exp = br.expected_entries(x, T["left1"], T["right1"], dec, T["size_int"], T["node_first"], T["leaf_pos"], T["ibox1"], leaf_box)
        for k in range(4):
            assert nodes[w, k, 7] == k, ("rank before the child order", w, k)
            if k >= len(exp):
                assert (nf[w, k, 0:6] == INF).all() and ni[w, k, 6] == rf.leaf_code(0, 1), ("empty slot", w, k)
                continue
            box, code, child = exp[k]
            assert same_bits(nf[w, k, 0:6], np.asarray(box, F)), ("entry box", w, k)
            if code is not None:
                assert ni[w, k, 6] == code, ("leaf code", w, k, int(ni[w, k, 6]), code)
                leaves.append(rf.leaf_range(code))
            else:
                c = int(ni[w, k, 6])
                assert 0 < c < N, ("child node index", w, k, c)
                referenced[c] += 1
                depth_of[c] = depth_of[w] + 1
                stack.append((c, child))
    assert visited == N and (referenced[1:] == 1).all() and referenced[0] == 0
    assert T["max_depth"] == depth_of.max()
    lf = T["level_first"]
    assert lf[0] == 0 and lf[-1] == N and len(lf) - 1 == T["num_levels"] == depth_of.max()
    for L in range(len(lf) - 1):
        assert (depth_of[lf[L]:lf[L + 1]] == L + 1).all(), ("level", L)
    # the leaf ranges tile the records
    leaves.sort()
    assert leaves[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(leaves, leaves[1:])) and leaves[-1][0] + leaves[-1][1] == T["num_refs"]
    assert all(1 <= c <= br.LEAF_MAX for _, c in leaves)


def check_build(name, p, cfg, T, mesh):
    ploc, budget, rounds, order = cfg
    n = p.shape[0]
    prim_of_ref, multi = check_splits(p, budget, T)
    R = T["num_refs"]
    boxes = T["boxes"]
    # ---- boxes and bounds
    if not T["have_splits"]:
        lo, hi = rf.tri_boxes(p)
        assert same_bits(boxes, np.concatenate([lo, hi], axis=1)), "boxes"
    assert same_bits(T["cbounds"], br.centroid_bounds(boxes[:, 0:3], boxes[:, 3:6])), ("centroid bounds", T["cbounds"])
    if T["tiny"]:
        check_tiny(p, T, mesh)
        return
    assert R > br.LEAF_MAX
    # ---- keys and sort
    ref, tree = reference_stages(name, boxes, ploc)
    assert (np.diff(T["keys_s"].astype(np.int64)) >= 0).all(), "keys_s descends"
    assert np.array_equal(T["keys_s"], ref["keys"][T["vals_s"]]), "a key is not its primitive's"
    assert np.array_equal(T["keys_s"], ref["ks"]) and np.array_equal(T["vals_s"], ref["vs"]), "not the stable sort"
    leaf_box, vals = ref["leaf_box"], ref["vs"]
    # ---- the binary tree as PLOC or Karras left it
    got = br.canonical(T["left0"], T["right0"], T["root"], T["ibox0"], vals)
    assert np.array_equal(got[0], tree["canonical"][0]), "leaf order of the binary tree"
    assert got[1].keys() == tree["canonical"][1].keys(), ("intervals of the binary tree", sorted(got[1].keys() ^ tree["canonical"][1].keys())[:8])
    assert got[1] == tree["canonical"][1], "boxes of the binary tree"
    if ploc:
        assert T["root"] == R - 2 and list(T["round_end"]) == tree["round_end"], ("round_end", list(T["round_end"]), tree["round_end"])
    else:
        assert T["root"] == 0
        assert same_bits(T["ibox0"], br.union_boxes(T["left0"], T["right0"], 0, leaf_box))
    # ---- the tree the collapse saw: after reinsertion still a binary tree over the same leaves, exact boxes, consistent shape
    size, first, leaf_pos, _ = br.shape_of(T["left1"], T["right1"], T["root"], R)
    assert np.array_equal(T["size_int"], size) and np.array_equal(T["node_first"], first) and np.array_equal(T["leaf_pos"], leaf_pos)
    assert same_bits(T["ibox1"], br.union_boxes(T["left1"], T["right1"], T["root"], leaf_box)), "a box is not the union of its children"
    if not (ploc and rounds > 0 and R > 16):
        assert not T["reinserted"]
    if not T["reinserted"]:
        assert np.array_equal(T["left1"], T["left0"]) and np.array_equal(T["right1"], T["right0"]) and same_bits(T["ibox1"], T["ibox0"])
    else:
        assert not (np.array_equal(T["left1"], T["left0"]) and np.array_equal(T["right1"], T["right0"])), "reinserted, but nothing moved"
    # ---- the programme
    dp = br.dp32(T["left1"], T["right1"], T["root"], size, T["ibox1"], leaf_box)
    bad = np.flatnonzero((dp != T["dp"]).any(axis=1))
    assert bad.size == 0, ("dp", bad[:8], dp[bad[:4]], T["dp"][bad[:4]])
    # ---- the emit
    check_wide_tree(T, T["root"], T["dp"][:, 3], leaf_box)
    # ---- the records
    prim_sorted = prim_of_ref[vals.astype(np.int64)]
    want = np.zeros((R, 12), np.uint32)
    want[leaf_pos] = rf.records(p[prim_sorted], prim_sorted, mesh[prim_sorted])
    assert same_bits(T["tris"], want), "records"
    assert np.array_equal(np.bincount(T["tris"][:, 9].astype(np.int64), minlength=n),
                          T["split_count"] if T["have_splits"] else np.ones(n, np.int64))
    # ---- the child order
    final = T["nodes"].reshape(-1, 4, 8)
    if not order:
        assert same_bits(T["nodes"], T["nodes_pre"]), "child order off, but the nodes changed"
    else:
        want = br.order_children(T["nodes_pre"], T["tris"], T["level_first"])
        bad = np.flatnonzero((want != T["nodes"]).any(axis=1))
        assert bad.size == 0, ("child order", bad[:8])
        live = final.view(F)[:, :, 0] < INF
        assert (live[:, :-1] | ~live[:, 1:]).all(), "an empty slot before a used one"
        assert (np.sort(final[:, :, 7], axis=1) == np.arange(4)).all(), "ranks are not a permutation of 0..3"
    if not T["have_splits"]:                                # (a reference's box holds its slab of the triangle, not the record)
        rf.check_conservative(T["nodes"], T["tris"], T["level_first"])


# ---- the tests -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,config", CASES)
def test_build_stages(hook, monkeypatch, name, config):
    ploc, budget, rounds, order = cfg = CONFIGS[config]
    tri = scene(name)
    p = tri.reshape(-1, 9)
    T = hook.debug_build(p, None, ploc=ploc, split_budget=budget, reinsert_rounds=rounds, order_children=order)
    print(name, config, "refs", T["num_refs"], "nodes", T["num_nodes"], "depth", T["max_depth"], "reinserted", T["reinserted"],
          "rounds", T["num_rounds"], "s_cut", T["s_cut"])
    check_build(name, p, cfg, T, np.zeros(p.shape[0], np.uint32))
    # the same hierarchy as fovpt_set_scene builds for these triangles under the same switches
    monkeypatch.setenv("FOVPT_BVH", "ploc" if ploc else "lbvh")
    monkeypatch.setenv("FOVPT_SPLIT", repr(budget))
    monkeypatch.setenv("FOVPT_REINSERT", str(rounds))
    monkeypatch.setenv("FOVPT_BVH_ORDER", "1" if order else "0")
    r = renderer.SampleRenderer(tc.model_of(tri))
    try:
        nodes, tris = hierarchy(r)
        st = r.stats()
    finally:
        r.close()
    assert (st.num_bvh_nodes, st.bvh_max_depth) == (T["num_nodes"], T["max_depth"])
    assert same_bits(tris[:T["num_refs"]], T["tris"]), "records differ from the scene's"
    assert wide_canonical(nodes, st.num_bvh_nodes) == wide_canonical(T["nodes"], T["num_nodes"]), "hierarchy differs from the scene's"


def test_mesh_ids_and_a_second_build_leave_no_trace(hook):
    """mesh_of_prim reaches the records; two builds of one scene give the same canonical hierarchy; bad switches are refused."""
    p = scene("soup65").reshape(-1, 9)
    mesh = (np.arange(p.shape[0]) % 3).astype(np.uint32)
    cfg = CONFIGS["ploc"]
    A = hook.debug_build(p, mesh, ploc=True)
    check_build("soup65", p, cfg, A, mesh)
    B = hook.debug_build(p, mesh, ploc=True)
    assert same_bits(A["tris"], B["tris"]) and wide_canonical(A["nodes"], A["num_nodes"]) == wide_canonical(B["nodes"], B["num_nodes"])
    from fovpathtracing_optixcodelatest_amd import lib
    for bad in (dict(split_budget=2.5), dict(split_budget=-1.0), dict(reinsert_rounds=-1)):
        with pytest.raises(lib.FovptError):
            hook.debug_build(p, None, **bad)


def test_reinsertion_lowers_the_cost_of_the_cards_scene(hook):
    """Slivers across a wall of small triangles: reinsertion changes the PLOC tree and the sum of its internal areas (binary64)
    falls.  Measured on gfx950: 3460.98 -> 3363.95 (2.80 % lower); the sequential reference of tests/test_build_stages_cpu.py
    reaches 3391.27 in 12 moves."""
    p = scene("cards").reshape(-1, 9)
    T = hook.debug_build(p, None, ploc=True, reinsert_rounds=REINSERT_DEFAULT)
    before, after = br.tree_cost64(T["ibox0"]), br.tree_cost64(T["ibox1"])
    print("cards: PLOC tree %.6g, reinserted %.6g (%.2f %% lower), reinserted = %d" % (before, after, 100 * (1 - after / before), T["reinserted"]))
    assert T["reinserted"] == 1 and after < before
    Z = hook.debug_build(p, None, ploc=True, reinsert_rounds=0)
    assert Z["reinserted"] == 0 and br.tree_cost64(Z["ibox1"]) == before
