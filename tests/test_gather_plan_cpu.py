"""The restated gather plan (tests/gather_ref.py) and its cases (tests/gather_cases.py), without a GPU: every case reaches what it
exists for -- measured here on the restated owner map, not taken from a table --, the plan is a partition in ascending order, it
agrees with the project's other statements of tile ownership, which get there by other routes (the painting resolve of
tests/resolve_ref.py, the launch-index owner of tests/generate_ref.py, multigpu.launch_owner / plan_from_owner_map), and the
restated pack / unpack are each other's inverse on the owned pixels and leave the holes alone."""
import numpy as np
import pytest

import gather_ref as gr
import generate_ref as gen
import reconstruct_ref as rc
import resolve_ref as rr
from fovpathtracing_optixcodelatest_amd import abi, multigpu

from gather_cases import BY_NAME, CASES, IDS, LOOP_WORDS, SMALL, random_words, restated


def test_the_case_list_is_the_one_the_tests_were_written_for():
    assert len(CASES) == len(BY_NAME) == 15
    assert all(c.uniform == (c.radii is None) and 1 <= c.world <= 64 for c in CASES)
    assert {c.name for c in CASES if c.size[0] * c.size[1] > 200 * 120} == {"chunked_scan", "long_pack", "long_unpack", "many_ranks_odd_tiles"}


# ---- every case reaches what it is for ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_reaches_what_it_is_for(case):
    owner, lists, counts = restated(case)
    s = gr.shape_of(owner, case.world)
    w, h = case.size
    pas, lx, ly = gr.launch_map(case.size, case.gaze, case.radii, case.uniform)
    want = dict(case.reaches)
    assert want, "a case without a purpose"
    for key in ("blocks", "per", "holes", "empty_ranks", "last_block", "scan_last", "owners_per_wave"):
        if key in want:
            assert s[key] == want.pop(key), (case.name, key, s[key])
    if "counts" in want:
        assert (min(counts), max(counts)) == want.pop("counts")
    if "exact_counts" in want:
        assert counts == want.pop("exact_counts")
    if "passes_seen" in want:
        assert sorted(int(p) for p in np.unique(pas) if p >= 0) == want.pop("passes_seen")
    if "max_owners_per_wave" in want:
        assert s["owners_per_wave"][1] == want.pop("max_owners_per_wave")
    if "full_wave_owners" in want:                                        # every wave of 64 pixels, the ragged last one aside
        flat = owner.reshape(-1)
        full = [len(np.unique(flat[b:b + 64])) for b in range(0, flat.size - 63, 64)]
        assert (min(full), max(full)) == want.pop("full_wave_owners") and full.count(max(full)) >= len(full) - 1
    if "periphery_grid" in want:
        P = rc.frame_passes(w, h, case.gaze, case.radii[0], case.radii[1], False)[0]
        assert (P[0], P[1]) == want.pop("periphery_grid")
    if "pack_words_above" in want:                                        # k_gather_pack's grid-stride loop turns
        assert max(counts) > want.pop("pack_words_above") == LOOP_WORDS
    if "unpack_words_above" in want:                                      # k_gather_unpack's does, and no single pack's
        assert sum(counts) > want.pop("unpack_words_above") == LOOP_WORDS > max(counts)
    if want.pop("fovea_only_on_last_row_and_column", False):
        y, x = np.nonzero(pas == 2)
        assert len(x) and ((x == w - 1) | (y == h - 1)).all()
        assert not (pas == 1).any()
        cx, cy = case.gaze
        assert cx - (case.radii[0] + 1) >= w and cy - (case.radii[0] + 1) >= h      # no launch index of the fovea pass lies in the frame
    if want.pop("owner_is_pass", False):                                  # one tile per pass: ownership rotates with the pass alone
        assert (lx[pas >= 0] < 128).all() and (ly[pas >= 0] < 64).all()
        assert np.array_equal(owner[pas >= 0], (pas[pas >= 0] % case.world).astype(np.uint8))
        assert [counts[p] > 0 for p in range(4)] == [True, True, True, False]
    if "same_plan_as" in want:
        other = restated(BY_NAME[want.pop("same_plan_as")])
        assert case.tile[0] <= 0 and case.tile[1] <= 0 and BY_NAME["holes"].tile is None
        assert np.array_equal(owner, other[0]) and counts == other[2]
        assert np.array_equal(owner, gr.owner_map(case.size, case.gaze, case.radii, case.uniform, case.world, (8, 4)))
    assert not want, "properties nobody checked: %s" % sorted(want)


def test_the_scan_cases_reach_every_branch_of_the_chunked_scan():
    """per == 1 with idle threads, per == 2 with a short last chunk and clamped threads behind it, per == 3 with full chunks."""
    def chunks(case):
        s = gr.shape_of(restated(case)[0], case.world)
        b0 = np.minimum(s["blocks"], np.arange(gr.SCAN_THREADS) * s["per"])
        b1 = np.minimum(s["blocks"], b0 + s["per"])
        return s["per"], b0, b1 - b0
    per, b0, n = chunks(BY_NAME["todays_frame"])
    assert per == 1 and (n[:94] == 1).all() and (n[94:] == 0).all()
    per, b0, n = chunks(BY_NAME["chunked_scan"])
    assert per == 2 and (n[:512] == 2).all() and n[512] == 1 and (n[513:] == 0).all() and (b0[513:] == 1025).all()      # (clamped)
    per, b0, n = chunks(BY_NAME["long_pack"])
    assert per == 3 and (n[:684] == 3).all() and (n[684:] == 0).all()
    # and a chunk's later blocks need more than the chunk's own offset: a rank owns pixels in two neighbouring blocks of one chunk
    for name in ("chunked_scan", "long_pack", "long_unpack", "many_ranks_odd_tiles"):
        case = BY_NAME[name]
        owner = restated(case)[0].reshape(-1)
        per, b0, n = chunks(case)
        seen = 0
        for t in np.flatnonzero(n >= 2):
            first, second = (owner[gr.BLOCK * (b0[t] + k):gr.BLOCK * (b0[t] + k + 1)] for k in (0, 1))      # blocks 0 and 1 of thread t's chunk
            both = np.intersect1d(first, second)
            seen += len(both[both != gr.NOBODY]) > 0
        assert seen >= 100, (name, seen)


# ---- the plan is a partition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_plan_is_an_ascending_partition_of_the_written_pixels(case):
    owner, lists, counts = restated(case)
    w, h = case.size
    fill = rc.writers(w, h, case.gaze, *(case.radii or (0, 0)), case.uniform)[0]
    assert len(lists) == len(counts) == case.world
    for r, a in enumerate(lists):
        assert len(a) == counts[r] and (np.diff(a) > 0).all()               # ascending, hence no index twice
        assert ((a >= 0) & (a < w * h)).all()
    every = np.concatenate(lists)
    assert len(np.unique(every)) == len(every)                              # disjoint
    assert np.array_equal(np.sort(every), np.flatnonzero(fill.reshape(-1) > 0))      # exactly the pixels with a writer
    assert ((owner == gr.NOBODY) == (fill == 0)).all() and (owner[fill > 0] < case.world).all()


# ---- agreement with the other restatements --------------------------------------------------------------------------------------------
def _config_and_params(case):
    cfg = abi.Config.reference_default()
    cfg.uniform = 1 if case.uniform else 0
    if not case.uniform:
        cfg.r_inner, cfg.r_outer = case.radii
    cfg.spp_periphery = cfg.spp_middle = cfg.spp_fovea = cfg.spp_uniform = 1
    lp = abi.LaunchParams()
    lp.frame.size.x, lp.frame.size.y = case.size
    lp.frame.c.x, lp.frame.c.y = case.gaze
    return cfg, lp


@pytest.mark.parametrize("case", SMALL, ids=[c.name for c in SMALL])
def test_rank_r_owns_what_the_sharded_resolve_writes_for_rank_r(case):
    """resolve_ref paints the frame launch by launch: a rank's own pixels get a colour, another rank's pixels zero, the pixels
    nobody writes keep what they held."""
    owner, lists, counts = restated(case)
    w, h = case.size
    cfg, lp = _config_and_params(case)
    passes = rr.render_passes(cfg, lp)
    slots, launches = rr.layout(passes)
    state = np.zeros(slots, np.uint32)
    cells, alpha, backplate = np.zeros((slots, 1, 4), np.float32), np.zeros((slots, 4), np.float32), np.zeros((launches, 4), np.float32)
    mine, kept = np.uint32(0xff010203), np.uint32(0x5a5a5a5a)
    ranks = range(case.world) if case.world <= 8 else sorted({0, 1, case.world // 2, case.world - 1})
    for rank in ranks:
        bufs = dict(accum=np.zeros((h, w, 4), np.float32), frame=np.full((h, w), kept, np.uint32))
        rr.resolve(passes, case.gaze, 1, 0, state, cells, alpha, backplate, bufs, lambda a: np.full(len(a), mine, np.uint32),
                   rank=rank, world=case.world, tile=gr.tile_of(case.tile))
        assert np.array_equal(np.flatnonzero(bufs["frame"].reshape(-1) == mine), lists[rank]), rank
        assert ((bufs["frame"] == kept) == (owner == gr.NOBODY)).all(), rank
        assert ((bufs["frame"] == 0) == ((owner != gr.NOBODY) & (owner != rank))).all(), rank


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_owner_is_generate_ref_owner_of_the_launch_index(case):
    owner = restated(case)[0]
    cfg, lp = _config_and_params(case)
    passes = rr.render_passes(cfg, lp)
    gen.job(passes)
    pas, lx, ly = gr.launch_map(case.size, case.gaze, case.radii, case.uniform)
    for p, P in enumerate(passes):
        sel = pas == p
        want = gen.owner(P, lx[sel], ly[sel], gr.tile_of(case.tile), case.world) if case.world > 1 else np.zeros(int(sel.sum()), np.int64)
        assert np.array_equal(owner[sel], want.astype(np.uint8)), p


@pytest.mark.parametrize("case", [c for c in CASES if c.uniform], ids=[c.name for c in CASES if c.uniform])
def test_uniform_frames_agree_with_multigpu(case):
    owner, lists, counts = restated(case)
    w, h = case.size
    y, x = np.mgrid[0:h, 0:w]
    own = multigpu.launch_owner(0, x, y, case.world, *gr.tile_of(case.tile)) + np.zeros((h, w), np.int64)
    assert np.array_equal(own, owner)
    got = multigpu.plan_from_owner_map(own, case.world)
    assert len(got) == case.world and all(np.array_equal(a, b) for a, b in zip(got, lists))
    got = multigpu.plan_from_owner_map(owner, case.world)                   # and with holes marked 255, which no uniform frame has
    assert all(np.array_equal(a, b) for a, b in zip(got, lists))


# ---- pack and unpack -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restated_pack_then_unpack_reproduces_a_frame_and_keeps_holes(case):
    owner, lists, counts = restated(case)
    npix = owner.size
    frame = random_words(npix, 11)
    for stride in {max(counts), (max(counts) + 63) // 64 * 64}:
        gathered = np.full(case.world * stride, 0xdeadbeef, np.uint32)
        for r in range(case.world):
            p = gr.pack(frame, lists, r)
            assert p.shape == (counts[r],)
            gathered[r * stride:r * stride + counts[r]] = p
        target = np.full(npix, 0x0badf00d, np.uint32)
        gr.unpack(gathered, stride, lists, target)
        written = owner.reshape(-1) != gr.NOBODY
        assert np.array_equal(target[written], frame[written])
        assert (target[~written] == 0x0badf00d).all()
