"""The references of the generate tests, checked without a device: the oracle's orc_camera_rays against whole oracle frames, the
restatement of tests/generate_ref.py against itself and against the cases of tests/generate_cases.py, the capacity of a queue
shard as a condition swept over the launches the library can make, and -- mutation by mutation -- that the cases can tell the
reference from a near miss.  tests/test_generate_gpu.py then holds the kernels to these references."""
import itertools

import numpy as np
import pytest

import generate_cases as gc
import generate_ref as gr
from fovpathtracing_optixcodelatest_amd import scenes
from gpu_common import bits

CASES = gc.cases()
BY_NAME = {c.name: c for c in CASES}
_expected = {}


def expected(oracle, case):
    if case.name not in _expected:
        _expected[case.name] = case.expected(oracle)
    return _expected[case.name]


@pytest.mark.parametrize("name", ["37x23_spp3_guides", "30x12_ring_5_10", "40x20_blocks_negative_offset", "257x3_spp1"])
def test_camera_rays_are_the_oracle_frames(oracle, name):
    """A max_depth = 1 launch over the Cornell box: the launch indices the frame traced are the entry's alive set, and the
    backplate every one of them ended with is the entry's, bit for bit."""
    case = BY_NAME[name]
    S = oracle.OracleScene(scenes.cornell_box())
    F = oracle.OracleFrame(case.size[0], case.size[1], oracle.HostProbe(gc.probe_data(case.probe)), scenes.CORNELL_CAMERA)
    case.set_params(F.lp)
    ps, slots, records = case.passes()
    P, rays = ps[0], case.camera_rays(oracle)[0]
    with oracle.SampleRecording(slots) as rec:
        oracle.launch(S, F, P.gw, P.gh, max_depth=1)
    rows = rec.rows
    assert len(rows["lx"]) == int(rays["alive"].sum()) * P.spp
    traced = np.zeros(P.gw * P.gh, bool)
    traced[rows["ly"] * P.gw + rows["lx"]] = True
    assert np.array_equal(traced, rays["alive"]) and 0 < traced.sum()
    last = rows["sample"] == P.spp - 1
    li = (rows["ly"] * P.gw + rows["lx"])[last]
    assert np.array_equal(bits(rows["backplate"][last]), bits(rays["backplate"][li]))
    # (the recorder keeps the backplate the sample left: of an earlier sample, that sample's own)
    assert np.isfinite(rays["dir"]).all() and np.isfinite(rays["backplate"]).all()


def test_no_case_makes_a_direction_that_is_not_finite(oracle):
    for case in CASES:
        for r in case.camera_rays(oracle):
            assert np.isfinite(r["dir"]).all() and np.isfinite(r["backplate"]).all(), case.name
            assert np.allclose(np.linalg.norm(r["dir"].astype(np.float64), axis=-1), 1.0, atol=1e-5), case.name


def test_ring_cases_hit_their_edges(oracle):
    """Some launch index lies at exactly r_inner, another at exactly r_outer, and both pass the ring test: the case builder asserts
    it from the oracle's ranges (Case.camera_rays) whenever such a case is built; here it is built, and the gaze itself is one."""
    ringed = [c for c in CASES if c.edges is not None]
    assert sorted(c.edges for c in ringed) == [(True, False), (True, True), (True, True)]
    for case in ringed:
        case.camera_rays(oracle)
    case = BY_NAME["30x12_ring_0_10"]
    P, rays = case.passes()[0][0], case.camera_rays(oracle)[0]
    assert 5 * P.gw + 10 in gc.ring_edge_indices(P, rays)[0] and rays["range"][5 * P.gw + 10] == 0.0   # the gaze: range 0 == r_inner
    # a gaze outside the frame or in its corner: some launch indices sit at wrapped pixel indices
    for name in ("101x67_fov_gaze_outside", "96x64_fov_corner_guides", "40x20_blocks_negative_offset"):
        wrapped = [int((r["pixel"] > 0x7fffffff).any(axis=1).sum()) for r in BY_NAME[name].camera_rays(oracle)]
        assert sum(wrapped) > 0, name
    r = BY_NAME["101x67_fov_gaze_outside"].camera_rays(oracle)
    assert any((x["alive"] & (x["pixel"] > 0x7fffffff).any(axis=1)).any() for x in r), "no live launch index at a wrapped pixel index"


def test_slots_are_a_permutation_and_kernels_are_the_ones_the_cases_are_for(oracle):
    for case in CASES:
        ex = expected(oracle, case)
        assert (ex["pass_of"] >= 0).all()                                                     # every slot is some (pass, li, s): expected() asserts "once"
        assert np.array_equal(ex["live"], ex["live_general"]), case.name                     # the padded walk reaches each owned live slot, once
        assert ex["count"].sum() == len(ex["live"]) and ex["count"].max() <= ex["cap"], case.name
        if case.kernel is not None:
            assert ex["kernel"] == case.kernel, (case.name, ex["kernel"])
        else:
            assert ex["kernel"] == 0
        if case.world > 1 and ex["kernel"] == 1:                                              # each owned launch index exactly once, all else padding
            ps, slots, _ = case.passes()
            p_, lx, ly, s, slot, it = gr.walk_owned(ps, case.rank, case.world, case.tiles())
            assert len(np.unique(slot)) == len(slot)
            mine = np.zeros(slots, bool)
            for P in ps:
                idx = gr.launch_indices(P).astype(np.int64)
                own = gr.owner(P, idx[:, 0], idx[:, 1], case.tiles(), case.world) == case.rank
                for k in range(P.spp):
                    mine[gr.slot_of(P, idx[own, 0], idx[own, 1], k)] = True
            assert np.array_equal(np.sort(slot), np.flatnonzero(mine)), case.name


def _frames():
    out = {}
    for case in CASES:
        out.setdefault(case.frame, []).append(case)
    return out


def test_ranks_and_chains_partition_their_frame(oracle):
    seen_ranks = seen_chains = 0
    for frame, members in _frames().items():
        whole = [c for c in members if c.world == 1 and c.chain is None and c.sel == 0]
        if len(members) == 1:
            continue
        assert len(whole) >= 1, frame
        base = expected(oracle, whole[0])
        for key, group in itertools.groupby(sorted((c for c in members if c.world > 1), key=lambda c: (c.world, c.tile, c.rank)),
                                            key=lambda c: (c.world, c.tile)):
            group = list(group)
            assert [c.rank for c in group] == list(range(key[0])), (frame, key)
            lives = [expected(oracle, c)["live"] for c in group]
            both = np.concatenate(lives)
            assert len(np.unique(both)) == len(both), (frame, key, "two ranks own one slot")
            assert np.array_equal(np.sort(both), base["live"]), (frame, key)
            seen_ranks += 1
        chains = [c for c in members if c.chain is not None or c.sel != 0]
        for pair in (("chain0", "chain1"), ("chain0_grid4", "chain1_grid4"), ("sel1_to_8231", "sel2_from_8231")):
            two = [c for c in chains if c.name.endswith(pair)]
            if two:
                assert len(two) == 2
                a, b = (expected(oracle, c) for c in two)
                assert a["slot_end"] == b["slot_begin"] and a["slot_begin"] == 0 and b["slot_end"] == base["slots"]
                assert not np.intersect1d(a["live"], b["live"]).size
                assert np.array_equal(np.union1d(a["live"], b["live"]), base["live"])
                assert set(np.unique(a["shard"][a["live"]])) <= {0, 1, 2, 3} and set(np.unique(b["shard"][b["live"]])) <= {4, 5, 6, 7}
                seen_chains += 1
    assert seen_ranks >= 16 and seen_chains == 3


def _sweep():
    """(passes as (gw, gh, spp) triples, rows, world, rank, tile, sel, grid): the launches a job can make -- grid a multiple of 8 (a
    chain: of 4), a chain's slots from generate_ref.chains, a sharded job one chain."""
    shapes = [[(gw, gh, spp)] for gw in (1, 3, 37, 130) for gh in (1, 7, 40) for spp in (1, 3, 16)]
    shapes += [[(24, 16, 1), (10, 10, 2), (8, 8, 3)], [(64, 64, 1), (7, 7, 1), (6, 6, 16)], [(1, 1, 8), (2, 2, 16), (1, 1, 32)]]
    for shape in shapes:
        rows = [None] + ([(5, 18)] if len(shape) == 1 and shape[0][1] == 40 else [])
        for r in rows:
            for world in (1, 2, 3, 5, 8):
                ranks = range(world) if world <= 3 else (0, world - 1)
                for rank in ranks:
                    for tile in ((8, 4), (5, 3)) if world > 1 else ((8, 4),):
                        for grid in (8, 64, gc.BIG_GRID):
                            yield shape, r, world, rank, tile, 0, grid
            for sel in (1, 2):
                for grid in (4, 8, 12, gc.BIG_GRID):
                    yield shape, r, 1, 0, (8, 4), sel, grid


def test_no_launch_the_library_can_make_overflows_a_shard():
    """shard_capacity(slots) = slots / 8 + 512 holds the entries of every shard, with every launch index alive, over a sweep of job
    shapes, grids (4, 8, 12, 64 blocks and more blocks than block iterations), chains, ranks and tiles.  (The test above states it
    for the cases, with their own ring tests, at the grid the case names or else at more blocks than block iterations, which is
    what a device's grid is to jobs this small; tests/test_generate_gpu.py states it again at the grid the device used.)"""
    n = 0
    for shape, rows, world, rank, tile, sel, grid in _sweep():
        ps = [gr.Pass(gw, gh, (1, 1), 1, (0, 0), 0.0, 1e9, spp, 0, 0) for gw, gh, spp in shape]
        slots, records = gr.job(ps, rows)
        b, e = (0, slots) if sel == 0 else gr.chains(slots)[sel - 1][1:]
        alive = [np.ones(P.gw * (P.row1 - P.row0), bool) for P in ps]
        ex = gr.expected(ps, slots, records, alive, rank=rank, world=world, tile=tile, sel=sel, slot_begin=b, slot_end=e, grid=grid)
        assert ex["count"].max() <= ex["cap"], (shape, rows, world, rank, tile, sel, grid, ex["count"].tolist(), ex["cap"])
        assert np.array_equal(ex["live"], ex["live_general"]), (shape, rows, world, rank, tile)
        n += 1
    assert n >= 2000, n


def _canonical(ex):
    return (np.int64(ex["kernel"]), ex["live"], ex["shard"], ex["count"], bits(ex["rng"]), bits(ex["dir"]), bits(ex["backplate"]), ex["record_live"])


def _differs(a, b):
    return any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(_canonical(a), _canonical(b)))


ORACLE_MUTATIONS = ("jy_first", "skip_one_draw", "random_late", "first_backplate", "signed_index", "inner_edge_dead")


@pytest.mark.parametrize("mutation", ORACLE_MUTATIONS + gr.MUTATIONS)
def test_the_cases_tell_a_near_miss_from_the_reference(oracle, mutation):
    """jy drawn before jx; one draw skipped per earlier sample; Random(seed) taken after the jitter draws; the first sample's
    backplate; the pixel index without the offset's wrap; range <= r_inner dead; the launch record not chunk-relative; the owner
    rotation without the frame pass; ty instead of 3 ty; the owned slot without - row0: each changes what some case expects."""
    caught = []
    for case in CASES:
        ref = expected(oracle, case)
        got = case.expected(oracle, variant=mutation) if mutation in ORACLE_MUTATIONS else case.expected(oracle, mut=mutation)
        if _differs(ref, got):
            caught.append(case.name)
            if len(caught) >= 3:
                break
    print(mutation, "changes what is expected of", caught)
    assert caught, "no case can tell %s from the reference" % mutation
