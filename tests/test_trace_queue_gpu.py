"""k_traverse's queue side ray by ray (fovpt_debug_trace_queued): the production closest-hit and occlusion launches on the queue
states of tests/trace_queue_cases.py -- rays spread over the shards of either queue in different layouts, shuffled sample slots,
all three radiance cells and alpha as targets, other iterations' counter words, one and two units of 256 threads and the
production grids, the two chains of a split frame beside each other.

The reference per ray is the oracle's brute force over all triangles (OracleScene.trace(..., brute=True)), and everything is
compared as bits.  Where a result must lie follows from the case's counts alone (trace_queue_cases.places): the test restates
no index formula of the library.  Whatever a launch must not write has to keep the hook's fill pattern -- the rest of the hit
buffer, every other cell, the trap slot of the idle queue entries, the other chain's shards and slots -- and the queues and
every counter word must be what was uploaded.  tests/test_trace_queue_cpu.py shows which branches the launches reach."""
import ctypes as C

import numpy as np
import pytest

import trace_cases as tc
import trace_queue_cases as qc
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer

pytestmark = pytest.mark.gpu

FILL = np.frombuffer(bytes([abi.DEBUG_SHADE_FILL] * 4), np.uint32)[0]
MISS = 0xFFFFFFFF


@pytest.fixture(scope="module")
def gpu():
    rs = {}
    for scene in qc.SCENES:
        r = renderer.SampleRenderer(tc.model_of(qc.batch(scene)[0]))
        cfg = abi.Config.reference_default()
        cfg.max_depth = qc.MAX_DEPTH
        r.config = cfg
        rs[scene] = r
    yield rs
    for r in rs.values():
        r.close()


@pytest.fixture(scope="module")
def truth(oracle):
    """The oracle's brute force over each scene's whole batch, once: (prim, tuv, occluded)."""
    out = {}
    for scene in qc.SCENES:
        tri, o, d = qc.batch(scene)
        out[scene] = oracle.OracleScene(tc.model_of(tri)).trace(o, d, brute=True)
    return out


@pytest.fixture(scope="module")
def plain(gpu):
    """The same batches through the unchanged fovpt_debug_trace: the secondary reference."""
    return {scene: gpu[scene].debug_trace(*qc.batch(scene)[1:]) for scene in qc.SCENES}


def _launch(r, run, mine, other, both=False):
    oth = dict(other, q_count=run.other_counts, sq_count=run.other_counts) if other is not None else None
    return r.debug_trace_queued(mine, run.q_count, run.sq_count, sel=run.sel, it_closest=run.iters[0], it_shadow=run.iters[1],
                                grid_closest=run.grid_closest, grid_shadow=run.grid_shadow, slots=run.slots, decoy=qc.DECOY, other=oth, both=both)


def check(name, run, launched, n_slots, got, want, plain):
    """What the launches left against the references.  launched: (rays, radiance counts) per chain that ran; n_slots: the sample
    slots of the state without the trap slot; want, plain: (prim, tuv, occluded) of the scene's batch."""
    cap = got["cap"]
    if run.layout == "brim":
        assert cap == 513
    pick = np.concatenate([rays["pick"] for rays, _ in launched])
    n = len(pick)
    wp, wt, wo = (x[pick] for x in want)
    # ---- the hit buffer: exactly the places of the launched rays, from the counts alone
    shard, entry = (np.concatenate(x) for x in zip(*[qc.places(counts) for _, counts in launched]))
    assert (entry < cap).all()
    place = shard.astype(np.int64) * cap + entry
    order = np.argsort(place)
    got_place = got["hit"]["shard"].astype(np.int64) * cap + got["hit"]["pos"]
    assert got["hit_found"] == n and np.array_equal(got_place, place[order]), (
        name, "hit records", got["hit_found"], n, np.setxor1d(got_place, place)[:8].tolist())
    ray = np.arange(n)[order]                          # the ray whose record the k-th entry found must be
    rec = got["hit"]["rec"]
    bad = np.flatnonzero(got["hit"]["prim"] != wp[ray])
    assert bad.size == 0, (name, "primitive of rays", ray[bad[:8]].tolist(), got["hit"]["prim"][bad[:8]], wp[ray][bad[:8]])
    hit = wp[ray] != MISS
    bad = np.flatnonzero((rec[:, :3].view(np.uint32) != wt[ray].view(np.uint32)).any(axis=1) & hit)
    assert bad.size == 0, (name, "t, u, v bits of rays", ray[bad[:8]].tolist(), rec[bad[:8]], wt[ray][bad[:8]])
    bad = np.flatnonzero((rec[:, 3].copy().view(np.uint32) != MISS) & ~hit)
    assert bad.size == 0, (name, "position word of missing rays", ray[bad[:8]].tolist())
    # ---- cells and alpha: (slot, target) of every launched ray holds the record the oracle's answer picks, xyz and +0
    want_cells = np.full((n_slots + 1, qc.MAX_DEPTH, 4), FILL, np.uint32)
    want_alpha = np.full((n_slots + 1, 4), FILL, np.uint32)
    slot = np.concatenate([rays["slot"] for rays, _ in launched]).astype(np.int64)
    target = np.concatenate([rays["target"] for rays, _ in launched])
    vis, occ = (np.concatenate([rays[k] for rays, _ in launched]) for k in ("vis", "occ"))
    value = np.where(wo.astype(bool)[:, None], occ, vis).astype(np.float32).view(np.uint32).copy()
    value[:, 3] = 0                                    # the bits of +0
    a = target == qc.ALPHA
    want_alpha[slot[a]] = value[a]
    want_cells[slot[~a], target[~a].astype(np.int64)] = value[~a]
    bad = np.argwhere((got["cells"].view(np.uint32) != want_cells).any(axis=2))
    assert bad.size == 0, (name, "cells (slot, cell)", bad[:8].tolist(), "rays", [np.flatnonzero(slot == s).tolist() for s in bad[:8, 0]])
    bad = np.flatnonzero((got["alpha"].view(np.uint32) != want_alpha).any(axis=1))
    assert bad.size == 0, (name, "alpha of slots", bad[:8].tolist(), "rays", [np.flatnonzero(slot == s).tolist() for s in bad[:8]])
    # ---- counters and queues
    assert (got["stat_radiance"], got["stat_shadow"]) == (n, n), (name, got["stat_radiance"], got["stat_shadow"], n)
    assert got["stat_paths"] == (n if run.iters[0] == 0 else 0), (name, got["stat_paths"])
    assert got["counters_changed"] == 0, (name, "counter words changed", got["counters_changed"])
    assert got["queues_unchanged"] == 1, (name, "a queue was written")
    # ---- secondary: the same rays through fovpt_debug_trace
    pp, pt, po = (x[pick] for x in plain)
    assert np.array_equal(got["hit"]["prim"], pp[ray]), (name, "primitive against fovpt_debug_trace")
    assert np.array_equal(rec[:, :3].view(np.uint32)[hit], pt[ray].view(np.uint32)[hit]), (name, "t, u, v against fovpt_debug_trace")
    assert np.array_equal(po.astype(bool), wo.astype(bool)), (name, "occlusion against fovpt_debug_trace")


@pytest.mark.parametrize("layout", list(qc.LAYOUTS))
@pytest.mark.parametrize("scene", sorted(qc.SCENES))
def test_layouts(gpu, truth, plain, scene, layout):
    """Every launch of a layout: the row as the radiance queue and as the shadow queue, iterations and grids by the run list.  A
    chain runs ALONE here, beside the other chain's live rays: their four shards of the hit buffer and all their slots keep the
    fill."""
    mine, other = qc.rays_of(scene, layout)
    mine_runs = [run for run in qc.runs() if run.layout == layout]
    assert len(mine_runs) >= 2
    for run in mine_runs:
        got = _launch(gpu[scene], run, mine, other)
        check((scene, run.name), run, [(mine, run.q_count)], run.n + run.n_other, got, truth[scene], plain[scene])


@pytest.mark.parametrize("layout", ["chain1", "chain2"])
@pytest.mark.parametrize("scene", sorted(qc.SCENES))
def test_both_chains_on_one_state(gpu, truth, plain, scene, layout):
    """sel = 1 and sel = 2 one after the other on the same state and stream: the union of what each leaves alone -- both ray sets
    complete, nothing else written."""
    mine, other = qc.rays_of(scene, layout)
    for run in (r for r in qc.runs() if r.layout == layout):
        got = _launch(gpu[scene], run, mine, other, both=True)
        check((scene, run.name, "both"), run, [(mine, run.q_count), (other, run.other_counts)], run.n + run.n_other, got, truth[scene], plain[scene])


def test_the_hook_refuses_bad_arguments(gpu, truth, plain):
    r = gpu["cornell"]
    E_INVALID, E_NO_SCENE = -1, -3
    mine, other = qc.rays_of("cornell", "chain1")
    run = qc.Run("chain1", False, (0, 0), 1, 1)

    def call(rays=mine, oth=other, **kw):
        a = dict(q_count=run.q_count, sq_count=run.sq_count, sel=1, it_closest=0, it_shadow=0, grid_closest=1, grid_shadow=1,
                 other=dict(oth, q_count=run.other_counts, sq_count=run.other_counts) if oth is not None else None)
        a.update(kw)
        return r.debug_trace_queued(rays, a.pop("q_count"), a.pop("sq_count"), **a)

    def with_(rays, **kw):
        return dict(rays, **kw)

    twice = mine["slot"].copy()
    twice[1] = twice[0]
    bad_target = mine["target"].copy()
    bad_target[2] = qc.MAX_DEPTH
    for kw in (dict(q_count=(17, 0, 5, 29, 0, 0, 0, 0)),                        # counts that do not sum to n
               dict(sq_count=(17, 0, 6, 30, 0, 0, 0, 0)),
               dict(q_count=(17, 0, 5, 0, 30, 0, 0, 0)),                        # counts outside sel
               dict(sel=2),
               dict(sel=3),
               dict(sel=0),                                                     # another chain's rays without chains
               dict(rays=with_(mine, slot=twice)),                              # no permutation
               dict(rays=with_(mine, slot=mine["slot"] + 1)),
               dict(oth=with_(other, slot=other["slot"] - 1)),
               dict(rays=with_(mine, target=bad_target)),                       # a target outside the range
               dict(it_closest=-1), dict(it_closest=63), dict(it_shadow=-1), dict(it_shadow=63),
               dict(grid_closest=-1), dict(decoy=(0, 0, 0, 0, 0, 0, 0, 1 << 20))):
        with pytest.raises(lib.FovptError) as err:
            call(**kw)
        assert err.value.code == E_INVALID, kw
    brim = qc.rays_of("cornell", "brim")[0]                                      # a count above cap = 513
    with pytest.raises(lib.FovptError) as err:
        r.debug_trace_queued(brim, (514, 0, 0, 513, 0, 0, 2, 513), qc.LAYOUTS["brim"][1], slots=8)
    assert err.value.code == E_INVALID
    L = r._L
    launch, res = abi.DebugTraceLaunch(), abi.DebugTraceResult()
    assert L.fovpt_debug_trace_queued(None, C.byref(launch), C.byref(res)) == E_INVALID
    assert L.fovpt_debug_trace_queued(r._ctx, None, C.byref(res)) == E_INVALID
    assert L.fovpt_debug_trace_queued(r._ctx, C.byref(launch), None) == E_INVALID
    launch.n, launch.q_count[0], launch.sq_count[0] = 1, 1, 1
    assert L.fovpt_debug_trace_queued(r._ctx, C.byref(launch), C.byref(res)) == E_INVALID         # null arrays
    bare = C.c_void_p()
    lib.check(None, L.fovpt_create(C.byref(bare), 0))
    try:
        launch.n, launch.q_count[0], launch.sq_count[0] = 0, 0, 0
        assert L.fovpt_debug_trace_queued(bare, C.byref(launch), C.byref(res)) == E_NO_SCENE
    finally:
        L.fovpt_destroy(bare)
    # n = 0 is a launch over empty queues, and a good call still works afterwards
    none = {k: v[:0] for k, v in mine.items()}
    got = r.debug_trace_queued(none, (0,) * 8, (0,) * 8)
    assert got["hit_found"] == 0 and got["counters_changed"] == 0 and got["queues_unchanged"] == 1
    assert (got["cells"].view(np.uint32) == FILL).all() and (got["alpha"].view(np.uint32) == FILL).all()
    check("after the refusals", run, [(mine, run.q_count)], run.n + run.n_other, call(), truth["cornell"], plain["cornell"])
