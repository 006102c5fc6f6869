"""k_shade on chosen hits (fovpt_debug_shade): the production kernel, launched once as a job launches it, against the oracle's
traceRadiance run from just behind trace_closest with the occlusion outcome given (oracle.shade_hit), mapped onto the
library's state by tests/shade_hit_ref.py -- whose docstring holds the rules.  Everything is compared as bits, NaN for NaN,
with the oracle in detmath mode; whatever a hit must not write has to keep the hook's fill pattern.

The ONE exemption: throughput, rayEta and the generator's words are compared only for hits that send a next ray -- nothing
reads them otherwise and the kernel leaves them stale; shade_hit_ref.expected() asserts that every other hit is DONE, at the
last depth or ended by the roulette.

The compaction is checked on every launch: the entries found anywhere in the next queue and the shadow queue are exactly the
expected ones (none lost, none twice), all of them inside the counted ranges of the selected shards, and no other counter
word changed; with one block and at most 256 hits the order is fixed as well.  tests/test_shade_hits_cpu.py shows which
branches the hits reach."""
import ctypes as C

import numpy as np
import pytest

import shade_hit_cases as hc
import shade_hit_ref as ref
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer

pytestmark = pytest.mark.gpu

FILL = np.frombuffer(bytes([abi.DEBUG_SHADE_FILL] * 4), np.uint32)[0]


@pytest.fixture(scope="module")
def gpu():
    rs = {c: renderer.SampleRenderer(hc.model(c)[0]) for c in (False, True)}
    yield rs
    for r in rs.values():
        r.close()


@pytest.fixture(scope="module")
def scenes_(oracle):
    return {c: oracle.OracleScene(hc.model(c)[0]) for c in (False, True)}


def _configure(r, probe, options, guides):
    cfg = abi.Config.reference_default()
    cfg.max_depth, cfg.options, cfg.write_guides = hc.MAX_DEPTH, options, guides
    r.config = cfg
    hc.probes()[probe].install(r)


def _bad(got, want):
    """Rows that differ: bit-equal, or NaN where the oracle has NaN."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    nan = np.isnan(want)
    bad = np.where(nan, ~np.isnan(got), got.view(np.uint32) != want.view(np.uint32))
    return bad.reshape(bad.shape[0], int(np.prod(bad.shape[1:]))).any(axis=1)


def _none(what, bad, *show):
    idx = np.flatnonzero(bad)
    assert idx.size == 0, (what, len(idx), "hits", idx[:6].tolist()) + tuple(s[idx[:3]] for s in show)


def _queue(what, n, found, count, q, sel, cap):
    """The entries found are inside the counted ranges of the selected shards, and no two share a place -> their slots."""
    assert found == int(count.sum()) and found <= n, (what, found, count.tolist())
    first, m = (4, 4) if sel == 2 else (0, 8 if sel == 0 else 4)
    assert not count[:first].any() and not count[first + m:].any(), (what, "outside the selection", count.tolist())
    assert (q["pos"] < count[q["shard"]]).all() and (count <= cap).all(), (what, "outside the counted ranges")
    place = q["shard"].astype(np.int64) * cap + q["pos"]
    assert len(np.unique(place)) == len(place)
    return q["o"][:, 3].copy().view(np.uint32)


def check(name, h, e, got, sel, guides):
    n = len(h["prim"])
    D = hc.MAX_DEPTH
    idx = np.arange(n)
    assert got["counters_changed"] == 0, name
    # ---- per slot
    _none((name, "flags | depth"), got["rng"][:, 2] != e["state"], got["rng"][:, 2], e["state"], h["note"])
    _none((name, "rng.w"), got["rng"][:, 3] != 0)
    nx = e["next"]
    _none((name, "generator of a hit that goes on"), nx & (got["rng"][:, :2] != e["rng"]).any(axis=1))
    _none((name, "throughput / rayEta of a hit that goes on"), nx & _bad(got["thr"], e["thr"]), got["thr"], e["thr"])
    want_rad = np.full((n, D, 4), 0, np.uint32)
    want_rad[...] = FILL
    want_rad = want_rad.view(np.float32)
    has = e["cell"] >= 0
    want_rad[idx[has], e["cell"][has], :3] = e["cell_value"][has]
    want_rad[idx[has], e["cell"][has], 3] = 0.0
    _none((name, "radiance cells"), _bad(got["rad"], want_rad), got["rad"], want_rad, e["cell"])
    want_alpha = np.full((n, 4), FILL, np.uint32).view(np.float32)
    want_alpha[e["alpha_set"], :3] = e["alpha_value"][e["alpha_set"]]
    want_alpha[e["alpha_set"], 3] = 0.0
    _none((name, "alpha"), _bad(got["alpha"], want_alpha), got["alpha"], want_alpha)
    for k, key in (("guide_n", "guide_n"), ("guide_a", "guide_a")):
        want = np.full((n, 4), FILL, np.uint32).view(np.float32)
        if guides:
            want[e["guide"], :3] = e[key][e["guide"]]
            want[e["guide"], 3] = 0.0
        _none((name, k), _bad(got[k], want), got[k], want)
    # ---- the next queue: exactly the expected rays, each once
    slots = _queue((name, "next"), n, got["next_found"], got["next_count"], got["next"], sel, got["cap"])
    order = np.argsort(slots, kind="stable")
    assert np.array_equal(slots[order], idx[nx]), (name, "next rays", len(slots), int(nx.sum()), np.setxor1d(slots, idx[nx])[:8].tolist())
    _none((name, "next origin"), _bad(got["next"]["o"][order][:, :3], e["next_o"][nx]))
    _none((name, "next direction, pdf"), _bad(got["next"]["d"][order], e["next_d"][nx]), got["next"]["d"][order], e["next_d"][nx])
    # ---- the shadow queue
    sh = e["shadow"]
    slots = _queue((name, "shadow"), n, got["shadow_found"], got["shadow_count"], got["shadow"], sel, got["cap"])
    order = np.argsort(slots, kind="stable")
    assert np.array_equal(slots[order], idx[sh]), (name, "shadow records", len(slots), int(sh.sum()), np.setxor1d(slots, idx[sh])[:8].tolist())
    s = {k: v[order] for k, v in got["shadow"].items()}
    _none((name, "shadow origin"), _bad(s["o"][:, :3], e["shadow_o"][sh]))
    _none((name, "shadow direction"), _bad(s["d"][:, :3], e["shadow_d"][sh]))
    _none((name, "shadow target"), s["d"][:, 3].copy().view(np.uint32) != e["shadow_target"][sh])
    zero = np.zeros((int(sh.sum()), 1), np.float32)
    _none((name, "val_vis"), _bad(s["vis"], np.concatenate([e["shadow_vis"][sh], zero], axis=1)))
    _none((name, "val_occ"), _bad(s["occ"], np.concatenate([e["shadow_occ"][sh], zero], axis=1)))


def _run(r, h, **kw):
    return r.debug_shade(h["origin"], h["dir"], h["prim"], h["tuv"], h["rng"], h["thr"], **kw)


@pytest.mark.parametrize("cfg", hc.CONFIGS, ids=lambda c: c[0])
def test_hits(oracle, gpu, scenes_, cfg):
    name, catcher, probe, options, guides = cfg
    h = hc.hits(catcher)
    n = len(h["prim"])
    vis, occ = ref.oracle_pair(oracle, scenes_[catcher], hc.probes()[probe].host_probe(oracle), hc.MAX_DEPTH, options, h)
    e = ref.expected(h, vis, occ, hc.MAX_DEPTH, catcher, guides)
    r = gpu[catcher]
    _configure(r, probe, options, guides)
    k = hc.CONFIGS.index(cfg)
    part, sel = k % 2, (0, 0, 1, 2)[k % 4]
    got = _run(r, h, depth_iter=k % 3, sel=sel, grid=8, partition=part, shard_count=hc.shard_counts(n, sel, "even"))
    print(name, n, "hits: next", int(e["next"].sum()), "shadow", int(e["shadow"].sum()), "cells", int((e["cell"] >= 0).sum()),
          "next per shard", got["next_count"].tolist())
    check(name, h, e, got, sel, guides)
    assert (got["next_count"] > 0).sum() == (8 if sel == 0 else 4)                 # several shards were filled


@pytest.fixture(scope="module")
def mixed(oracle, scenes_):
    """1000 hits of the catcher scene and what they must leave (probe sky96x40, no options)."""
    h = hc.subset(hc.hits(True), np.arange(1000))
    hp = hc.probes()["sky96x40"].host_probe(oracle)
    vis, occ = ref.oracle_pair(oracle, scenes_[True], hp, hc.MAX_DEPTH, 0, h)
    return h, ref.expected(h, vis, occ, hc.MAX_DEPTH, True, 0)


def _in_order(name, q, partition):
    """One block, at most 256 hits: ascending input order; with the partition all rays with dir.y <= 0 first."""
    slots = q["o"][:, 3].copy().view(np.uint32).astype(np.int64)
    assert (np.diff(q["shard"].astype(np.int64) * (1 << 32) + q["pos"]) > 0).all()
    if partition and "vis" not in q:
        up = q["d"][:, 1] > 0
        assert not (up[:-1] & ~up[1:]).any(), (name, "a ray of class 0 behind one of class 1")
        for cls in (up, ~up):
            assert (np.diff(slots[cls]) > 0).all(), (name, "class out of input order")
        assert len(up) < 16 or (up.any() and (~up).any())
    else:
        assert (np.diff(slots) > 0).all(), (name, "out of input order")


@pytest.mark.parametrize("case", hc.compaction_cases(), ids=lambda c: "n%d_grid%d_sel%d_%s_part%d" % c)
def test_compaction(gpu, mixed, case):
    n, grid, sel, spread, part = case
    h, e = mixed
    sub = np.arange(n)
    hs, es = hc.subset(h, sub), {k: v[sub] for k, v in e.items()}
    r = gpu[True]
    _configure(r, "sky96x40", 0, 0)
    got = _run(r, hs, depth_iter=2, sel=sel, grid=grid, partition=part, shard_count=hc.shard_counts(n, sel, spread))
    name = "n%d_grid%d_sel%d_%s_part%d" % case
    check(name, hs, es, got, sel, 0)
    if grid == 1 and n <= 256:
        _in_order(name, got["next"], part)
        _in_order(name, got["shadow"], part)
        if n >= 63:
            assert len(got["next"]["pos"]) > 8 and len(got["shadow"]["pos"]) > 8


@pytest.mark.parametrize("part", (0, 1))
def test_compaction_without_a_mix(gpu, mixed, part):
    """Each predicate all true and all false over a launch, and a whole wave without any entry between full ones."""
    h, e = mixed
    r = gpu[True]
    _configure(r, "sky96x40", 0, 0)
    both, neither = np.flatnonzero(e["next"] & e["shadow"]), np.flatnonzero(~e["next"] & ~e["shadow"])
    only_next, only_shadow = np.flatnonzero(e["next"] & ~e["shadow"]), np.flatnonzero(~e["next"] & e["shadow"])
    assert min(len(both), len(neither), len(only_next)) >= 64, (len(both), len(neither), len(only_next), len(only_shadow))
    picks = dict(all_both=both[:200], all_neither=neither[:200], next_only=only_next[:200],
                 empty_wave=np.concatenate([both[:64], neither[:64], only_next[:64], neither[64:128], both[64:70]]))
    if len(only_shadow) >= 8:
        picks["shadow_only"] = only_shadow[:200]
    for name, sub in picks.items():
        hs, es = hc.subset(h, sub), {k: v[sub] for k, v in e.items()}
        for grid in (1, 3):
            got = _run(r, hs, depth_iter=1, sel=0, grid=grid, partition=part)
            check((name, grid, part), hs, es, got, 0, 0)
            if grid == 1 and len(sub) <= 256:
                if len(got["next"]["pos"]) > 1 and not part:
                    _in_order(name, got["next"], 0)
                if len(got["shadow"]["pos"]) > 1:
                    _in_order(name, got["shadow"], 0)


def test_the_hook_refuses_bad_arguments(gpu, mixed):
    r = gpu[False]
    _configure(r, "sky96x40", 0, 0)
    h = hc.subset(mixed[0], np.flatnonzero(mixed[0]["prim"] == hc.NO_HIT)[:4])
    E_INVALID, E_NO_SCENE, E_NO_PROBE = -1, -3, -4
    good = _run(r, h)
    assert good["next_found"] == 0 and good["shadow_found"] == 0
    for kw in (dict(sel=3), dict(grid=0), dict(depth_iter=-1), dict(depth_iter=63), dict(shard_count=[1, 1, 1, 0, 0, 0, 0, 0]),
               dict(sel=1, shard_count=[0, 0, 0, 0, 4, 0, 0, 0]), dict(sel=2, shard_count=[4, 0, 0, 0, 0, 0, 0, 0])):
        with pytest.raises(lib.FovptError) as err:
            _run(r, h, **kw)
        assert err.value.code == E_INVALID, kw
    bad = dict(h, prim=np.full(4, 1 << 20, np.uint32))
    with pytest.raises(lib.FovptError) as err:
        _run(r, bad)
    assert err.value.code == E_INVALID
    with pytest.raises(lib.FovptError) as err:
        _run(r, h, probe=abi.Probe())
    assert err.value.code == E_NO_PROBE
    L = r._L
    launch, res = abi.DebugShadeLaunch(), abi.DebugShadeResult()
    assert L.fovpt_debug_shade(None, C.byref(r.launchParams.probe), C.byref(launch), None, None, None, None, None, None, C.byref(res)) == E_INVALID
    assert L.fovpt_debug_shade(r._ctx, C.byref(r.launchParams.probe), None, None, None, None, None, None, None, C.byref(res)) == E_INVALID
    launch.n = 1
    assert L.fovpt_debug_shade(r._ctx, C.byref(r.launchParams.probe), C.byref(launch), None, None, None, None, None, None, C.byref(res)) == E_INVALID
    bare = C.c_void_p()
    lib.check(None, L.fovpt_create(C.byref(bare), 0))
    try:
        launch.n, launch.grid = 0, 1
        assert L.fovpt_debug_shade(bare, C.byref(r.launchParams.probe), C.byref(launch), None, None, None, None, None, None, C.byref(res)) == E_NO_SCENE
    finally:
        L.fovpt_destroy(bare)
    # n = 0 is a launch over an empty queue, and a good call still works afterwards
    assert _run(r, hc.subset(h, np.arange(0)))["next_found"] == 0
    assert _run(r, h)["counters_changed"] == 0
