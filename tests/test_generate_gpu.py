"""k_generate and k_generate_owned on chosen frames (fovpt_debug_generate): the production launcher, as a job calls it on the
frame a render() or a launch() of the case's parameters would run, and everything the launch left -- the generator words, the
backplates, the guides, the queue counters and the entries of queue 0 -- against the oracle's camera rays (orc_camera_rays)
and the restatement of tests/generate_ref.py.  All comparisons are bitwise.  tests/test_generate_cpu.py ties the two
references to the oracle's frames and shows what the cases of tests/generate_cases.py can tell apart.

What generate must leave behind, whichever kernel made it:
  - queue 0 holds exactly the live slots (in the slot range, ring-alive, owned by the rank), each once, packed at [0, count[s]) of
    the shard the restatement assigns it (positions inside a shard are free), count[s] <= cap, no other counter touched;
  - an entry is (eye, slot as bits) and (the oracle's direction of that launch index and sample, 0);
  - rng of a live slot is (Random(seed) word 1, word 2, 0, 0); the backplate record of a launch index whose last sample is live
    is the oracle's; under write_guides the guides of a live slot are zero;
  - everything else -- the rng words and guides of other slots, the records of other launch indices, the rest of the queue -- is
    untouched."""
import ctypes as C

import numpy as np
import pytest

import generate_cases as gc
from common import cfg_uniform, make_gpu
from gpu_common import bits
from fovpathtracing_optixcodelatest_amd import abi, renderer, scenes

pytestmark = pytest.mark.gpu

FILL = np.frombuffer(bytes([abi.DEBUG_SHADE_FILL] * 4), np.uint32)[0]
CASES = gc.cases()


def _renderer():
    return renderer.SampleRenderer(scenes.cornell_box())


def _install(r, case):
    """The case's frame size, probe, configuration and launch parameters on the renderer."""
    r.resize(case.size)
    if getattr(r, "_generate_probe", None) != case.probe:
        r.setProbe(renderer.ProbeData(gc.probe_data(case.probe)).BuildCDF())
        r._generate_probe = case.probe
    r.config = case.config()
    case.set_params(r.launchParams)


def _run(r, case):
    _install(r, case)
    w, h = case.launch_grid()
    b, e = case.slot_range
    sel = case.sel if case.chain is None else case.chain + 1                 # a chain: the hook finds its slots itself
    return r.debug_generate(render=case.render is not None, width=w, height=h, rows=case.rows, sel=sel, slot_begin=b, slot_end=e, grid=case.grid)


def _check(oracle, case, out):
    ex = case.expected(oracle, grid=out["grid"])
    passes, slots, records = case.passes()
    live, count, cap = ex["live"], out["count"].astype(np.int64), out["cap"]
    print(case.name, "slots", slots, "live", len(live), "kernel", out["kernel"], "grid", out["grid"], "cap", cap, "count", count.tolist())
    assert [(p.gw, p.rows, p.spp, p.slot_base, p.launch_base) for p in out["passes"]] == \
           [(P.gw, P.row1 - P.row0, P.spp, P.slot_base, P.launch_base) for P in passes]
    assert (out["slot_begin"], out["slot_end"]) == (ex["slot_begin"], ex["slot_end"]) and cap == ex["cap"]
    assert out["kernel"] == ex["kernel"] and (case.kernel is None or out["kernel"] == case.kernel)
    if case.grid:
        assert out["grid"] == case.grid
    # found and count
    assert out["found"] == len(live), (case.name, out["found"], len(live))
    assert count.sum() == out["found"] and np.array_equal(count, ex["count"]), (case.name, count.tolist(), ex["count"].tolist())
    assert count.max() <= cap and out["counters_changed"] == 0
    # the queue entries
    shard, pos = out["shard"].astype(np.int64), out["pos"].astype(np.int64)
    assert (shard < 8).all(), "entries in the guard region behind the eighth shard"
    for s in range(8):
        assert np.array_equal(np.sort(pos[shard == s]), np.arange(count[s])), (case.name, "shard", s)
    slot = bits(out["o"][:, 3]).astype(np.int64)
    assert len(np.unique(slot)) == len(slot) and np.array_equal(np.sort(slot), live), case.name
    assert np.array_equal(shard, ex["shard"][slot]), (case.name, "a slot in another shard than its block iteration's")
    assert (bits(out["o"][:, :3]) == bits(ex["eye"])[None, :]).all()
    assert (bits(out["d"][:, 3]) == 0).all()
    assert np.array_equal(bits(out["d"][:, :3]), bits(ex["dir"][slot])), case.name
    # the generator words
    is_live = np.zeros(slots, bool)
    is_live[live] = True
    assert np.array_equal(out["rng"][live, :2], ex["rng"][live]) and (out["rng"][live, 2:] == 0).all(), case.name
    assert (out["rng"][~is_live] == FILL).all(), (case.name, "rng words of a slot that is not live were written")
    # the backplates
    rl = ex["record_live"]
    assert np.array_equal(bits(out["backplate"][rl, :3]), bits(ex["backplate"][rl])), case.name
    assert (out["backplate"][rl, 3] == 1.0).all()                                          # (the probe texel's own w)
    assert (bits(out["backplate"][~rl]) == FILL).all(), (case.name, "the record of a launch index without a live last sample was written")
    # the guides
    if case.guides:
        for g in (out["guide_n"], out["guide_a"]):
            assert (bits(g[live]) == 0).all() and (bits(g[~is_live]) == FILL).all(), case.name
    else:
        assert out["guide_n"] is None and out["guide_a"] is None
    return ex


def _group(oracle, group):
    """Runs the cases of a group on one renderer -> {case name: (case, hook output, expected)}."""
    r = _renderer()
    done = {}
    try:
        for case in CASES:
            if case.group == group:
                out = _run(r, case)
                done[case.name] = (case, out, _check(oracle, case, out))
    finally:
        r.close()
    return done


@pytest.mark.parametrize("group", ["uniform", "foveated", "chunks"])
def test_generate(oracle, group):
    done = _group(oracle, group)
    assert len(done) >= 5
    if group == "uniform":
        one_row = {gc.ONE_ROW[c.probe] for c, _, _ in done.values()}
        assert one_row == {True, False}


def _by_slot(out, ex):
    """The hook's output in slot order: direction of every live slot (zero elsewhere)."""
    d = np.zeros((ex["slots"], 4), np.float32)
    d[bits(out["o"][:, 3]).astype(np.int64)] = out["d"]
    return d


def test_chains(oracle):
    """The two chains of the smallest job that is split, as a job issues them (at its own grid and at four blocks) and at a split
    that is no multiple of 256: each leaves its half in its four shards, and together what the unsplit launch leaves."""
    done = _group(oracle, "chains")
    case, base, bex = done["128x128_uniform"]
    whole = _by_slot(base, bex)
    for a, b in (("128x128_chain0", "128x128_chain1"), ("128x128_chain0_grid4", "128x128_chain1_grid4"), ("128x128_sel1_to_8231", "128x128_sel2_from_8231")):
        (ca, oa, ea), (cb, ob, eb) = done[a], done[b]
        assert oa["slot_end"] == ob["slot_begin"] and set(oa["shard"].tolist()) <= {0, 1, 2, 3} and set(ob["shard"].tolist()) <= {4, 5, 6, 7}
        assert not ((ea["shard"] >= 0) & (eb["shard"] >= 0)).any()
        assert np.array_equal(bits(np.where((ea["shard"] >= 0)[:, None], _by_slot(oa, ea), _by_slot(ob, eb))), bits(whole))
        rng = np.where((ea["shard"] >= 0)[:, None], oa["rng"], ob["rng"])
        assert np.array_equal(rng, base["rng"])
    assert done["128x128_chain0"][1]["grid"] * 2 == base["grid"] and done["128x128_chain0"][1]["grid"] % 4 == 0


def test_sharded_frames(oracle):
    """Every rank of 2, 3, 4 and 8 over a launch and a three-pass frame, with both tile shapes: k_generate_owned leaves for each
    of its live slots what k_generate left for that slot in the world = 1 run of the frame, and the ranks' live slots are a
    partition of that run's.  A grid three launch indices wide makes the launcher fall back to k_generate."""
    done = _group(oracle, "sharded")
    frames = {}
    for case, out, ex in done.values():
        frames.setdefault(case.frame, []).append((case, out, ex))
    assert len(frames) == 3
    for frame, members in frames.items():
        base = [m for m in members if m[0].world == 1]
        assert len(base) == 1
        _, bout, bex = base[0]
        whole = _by_slot(bout, bex)
        owned_by = {}
        for case, out, ex in members:
            if case.world == 1:
                continue
            assert out["kernel"] == (0 if frame == "3x40" else 1), case.name
            live, rl = ex["live"], ex["record_live"]
            assert np.array_equal(bits(_by_slot(out, ex)[live]), bits(whole[live])), case.name
            assert np.array_equal(out["rng"][live], bout["rng"][live]), case.name
            assert np.array_equal(bits(out["backplate"][rl]), bits(bout["backplate"][rl])), case.name
            owned_by.setdefault((case.world, case.tile), []).append(live)
        for key, lives in owned_by.items():
            both = np.concatenate(lives)
            assert len(lives) == key[0] and len(np.unique(both)) == len(both) and np.array_equal(np.sort(both), bex["live"]), (frame, key)


def test_the_set_is_left_as_a_job_expects_it(oracle):
    """A frame rendered after the hook has used a state set is the frame rendered before, and lp is not changed."""
    size = (32, 32)
    r = make_gpu(scenes.cornell_box(), scenes.sky_probe(32, 16), scenes.CORNELL_CAMERA, size, cfg_uniform(2, 4))
    try:
        frames = []
        for k in range(4):
            r.launchParams.frame.subframe_index = 0
            r.render()
            frames.append((r.downloadAccum(), r.downloadPixels()))
            if k < 3:
                r.launchParams.frame.subframe_index = 3
                out = r.debug_generate()
                assert out["found"] == 32 * 32 * 2 and out["counters_changed"] == 0 and r.launchParams.frame.subframe_index == 3
        for a, p in frames[1:]:
            assert np.array_equal(a.view(np.uint32), frames[0][0].view(np.uint32)) and np.array_equal(p, frames[0][1])
    finally:
        r.close()


def test_the_hook_refuses_bad_arguments():
    E_INVALID, E_NO_PROBE, E_NO_FRAME = -1, -4, -5
    r = _renderer()
    try:
        L, ctx, lp = r._L, r._ctx, r.launchParams
        case = next(c for c in CASES if c.name == "37x23_spp1")
        passes, n, res = (abi.DebugPass * 3)(), C.c_int(0), abi.DebugGenerateResult()

        def call(lp_, launch, out=res, ctx_=ctx, passes_=passes):
            return L.fovpt_debug_generate(ctx_, C.byref(lp_) if lp_ is not None else None, C.byref(launch) if launch is not None else None, passes_,
                                          C.byref(n), C.byref(out) if out is not None else None)

        def launch(**kw):
            g = abi.DebugGenerateLaunch()
            g.render, g.width, g.height = 0, 37, 23
            for k, v in kw.items():
                setattr(g, k, v)
            return g

        r.resize(case.size)
        r.config = case.config()
        case.set_params(lp)
        assert call(lp, launch(), out=None) == E_NO_PROBE                                      # no probe yet
        r.setProbe(renderer.ProbeData(gc.probe_data("sky")).BuildCDF())
        assert call(lp, launch(), out=None) == 0 and n.value == 1 and (passes[0].gw, passes[0].rows, passes[0].spp) == (37, 23, 1)
        # a result with room for the launch's 851 slots and records: with it a call fails only for the reason under test
        slots = 37 * 23
        rooms = dict(rng4=np.zeros((slots, 4), np.uint32), backplate4=np.zeros((slots, 4), np.float32), place2=np.zeros((slots, 2), np.uint32),
                     o4=np.zeros((slots, 4), np.float32), d4=np.zeros((slots, 4), np.float32))
        full = abi.DebugGenerateResult()
        for k, v in rooms.items():
            setattr(full, k, v.ctypes.data)
        for good in (dict(), dict(grid=16), dict(sel=1, grid=4), dict(sel=2), dict(slot_begin=4, slot_end=5), dict(slot_end=851), dict(row0=5, row1=23)):
            assert call(lp, launch(**good), out=full) == 0, good
        assert full.found == (23 - 5) * 37 and full.cap == (23 - 5) * 37 // 8 + 512
        assert call(lp, launch()) == E_INVALID                                                 # a result without arrays
        # what is checked before the result is looked at: asked for the pass table alone (out = NULL), which a good call hands out
        assert call(lp, launch(), out=None) == 0
        assert call(lp, launch(), out=None, ctx_=None) == E_INVALID and call(None, launch(), out=None) == E_INVALID and call(lp, None, out=None) == E_INVALID
        assert call(lp, launch(), out=None, passes_=None) == E_INVALID
        bare = lp.copy()
        bare.frame.frame_buffer = None
        assert call(bare, launch(), out=None) == E_NO_FRAME
        zero = lp.copy()
        zero.samples_per_launch = 0
        assert call(zero, launch(), out=None) == E_INVALID
        for bad in (dict(row0=5, row1=24), dict(row0=7, row1=7), dict(row0=8, row1=7), dict(render=1, row1=3), dict(render=1, row0=1),
                    dict(width=1 << 16, height=1 << 16)):                                      # (the last: several jobs)
            assert call(lp, launch(**bad), out=None) == E_INVALID, bad
        # what is checked of the launch itself: the neighbours above succeed with the same result
        for why, bad in ((b"sel 3", dict(sel=3)), (b"grid of 12", dict(grid=12)), (b"grid of -8", dict(grid=-8)), (b"grid of 4", dict(grid=4)),
                         (b"grid of 6", dict(sel=1, grid=6)), (b"grid of 2", dict(sel=2, grid=2)), (b"slots [5, 4)", dict(slot_begin=5, slot_end=4)),
                         (b"slots [0, 852)", dict(slot_end=852)), (b"slots [852, 852)", dict(slot_begin=852, slot_end=852))):
            assert call(lp, launch(**bad), out=full) == E_INVALID, bad
            assert why in L.fovpt_last_error(ctx), (bad, L.fovpt_last_error(ctx))
        guided = case.config()
        guided.write_guides = 1                                 # guides wanted, no room given for them
        r.config = guided
        assert call(lp, launch(), out=full) == E_INVALID
        r.config = case.config()
        # a good call still works, and nothing of the parameters was changed
        out = r.debug_generate(render=False, width=37, height=23, sel=1, grid=4)
        assert out["found"] == 256 and (out["slot_begin"], out["slot_end"], out["grid"]) == (0, 256, 4) and out["count"].tolist() == [256, 0, 0, 0, 0, 0, 0, 0]
        assert lp.frame.subframe_index == case.subframe and lp.samples_per_launch == 1
    finally:
        r.close()
