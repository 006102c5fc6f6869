"""Without a GPU: the restatement of the resolve (tests/resolve_ref.py) is the oracle's, and the cases of tests/resolve_cases.py
reach what they are for.

The restatement is cross-checked on frames the oracle renders: the oracle records what every sample added (its radiance terms
in order, prd.alpha, the guides, the backplate); laid out as a path state in slot order and painted by resolve_ref they must
give the oracle's accum, rgba8 and guide buffers bit for bit -- with all three passes, a gaze in a corner, accumulate mode
against a history, overlapping fills and the opt-in sky term."""
import numpy as np
import pytest

import resolve_cases as rc
import resolve_ref as rr
from common import cfg_foveated, cfg_uniform, make_oracle
from fovpathtracing_optixcodelatest_amd import abi, scenes

PROBE = scenes.sky_probe(32, 16)


def _same_bits(what, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (what, len(bad), bad[:5].tolist())


def _state_from_rows(rows, passes, slots, launches, max_depth):
    """The oracle's per-sample terms as the library's path state."""
    state = np.full(slots, rc.DEAD_STATE, np.uint32)
    cells = np.full((slots, max_depth, 4), np.nan, np.float32)
    alpha = np.full((slots, 4), np.nan, np.float32)
    gn, ga = np.full((slots, 4), np.nan, np.float32), np.full((slots, 4), np.nan, np.float32)
    backplate = np.full((launches, 4), np.nan, np.float32)
    kinds = set()
    for i in range(len(rows["launch"])):
        P = passes[rows["launch"][i]]
        li = rows["ly"][i] * P.gw + rows["lx"][i]
        slot = P.slot_base + li * P.spp + rows["sample"][i]
        n = int(rows["nterm"][i])
        assert n <= max_depth
        a = rows["alpha"][i]
        flag = rr.ALPHA_ONE if (a == 1.0).all() else rr.ALPHA_SET if (a != 0.0).any() else 0
        kinds.add((n, flag))
        state[slot] = flag | (n << 8)
        cells[slot, :n, :3] = rows["terms"][i, :n]
        alpha[slot, :3] = a
        gn[slot, :3], ga[slot, :3] = rows["normal"][i], rows["albedo"][i]
        if rows["sample"][i] == P.spp - 1:
            backplate[P.launch_base + li, :3] = rows["backplate"][i]
    return dict(state=state, cells=cells, alpha=alpha, backplate=backplate, guide_n=gn, guide_a=ga), kinds


@pytest.mark.parametrize("name", ["fov_accumulate", "fov_gaze_corner", "uniform_guides", "fov_sky_miss", "launch_overlapping_accumulate"])
def test_the_restatement_paints_the_oracles_frames(oracle, name):
    size, gaze, sub = (40, 24), None, 0
    launch = None
    if name == "fov_accumulate":
        cfg, sub = cfg_foveated(3, 8, (1, 2, 3)), 2
        cfg.accumulate = 1
    elif name == "fov_gaze_corner":
        cfg, gaze = cfg_foveated(2, 6, (2, 1, 2), max_depth=2), (39, 23)
    elif name == "uniform_guides":
        cfg, size = cfg_uniform(2, 3), (24, 16)
        cfg.write_guides = 1
    elif name == "fov_sky_miss":
        cfg = cfg_foveated(3, 8, (1, 1, 2), max_depth=3)
        cfg.options = abi.OPT_SKY_MISS | abi.OPT_RUSSIAN_ROULETTE
    else:
        cfg, sub, size = cfg_uniform(1, 4), 3, (21, 9)
        cfg.accumulate = 1
        launch = dict(grid=(10, 4), factor=2, fill=4, offset=(1, 0), spp=2)
    S, F = make_oracle(oracle, scenes.cornell_box(), PROBE, scenes.CORNELL_CAMERA, size, gaze=gaze, subframe_index=sub)
    g = np.random.default_rng(5)
    F.accum[...] = g.random(F.accum.shape, np.float32) * np.float32(16.0) - np.float32(2.0)
    F.frame[...] = rc.FRAME_SENTINEL
    for b in (F.normal, F.color, F.albedo):
        b[...] = rc.GUIDE_SENTINEL
    bufs = dict(accum=F.accum.copy(), frame=F.frame.copy(), normal=F.normal.copy(), color=F.color.copy(), albedo=F.albedo.copy())
    if launch is not None:
        case = rc.Case(name, size, launch=launch, subframe=sub)
        case.set_params(F.lp)
        passes = rr.launch_pass(F.lp, *launch["grid"])
    else:
        passes = rr.render_passes(cfg, F.lp)
    slots, launches = rr.layout(passes)
    with oracle.SampleRecording(slots) as rec:
        if launch is not None:
            oracle.launch(S, F, launch["grid"][0], launch["grid"][1], max_depth=cfg.max_depth, accumulate=cfg.accumulate)
        else:
            oracle.render(S, F, cfg)
    st, kinds = _state_from_rows(rec.rows, passes, slots, launches, cfg.max_depth)
    print(name, "samples", len(rec.rows["launch"]), "(segments, alpha flag) seen:", sorted(kinds))
    assert len(kinds) >= 3
    gz = gaze if gaze is not None else (size[0] // 2, size[1] // 2)
    last = rr.resolve(passes, gz, cfg.max_depth, cfg.accumulate, st["state"], st["cells"], st["alpha"], st["backplate"], bufs, oracle.make_color,
                      guide_n=st["guide_n"] if cfg.write_guides else None, guide_a=st["guide_a"] if cfg.write_guides else None)
    if launch is None and not cfg.uniform:
        assert set(np.unique(last)) >= {0, 1, 2}
    _same_bits("accum", bufs["accum"], F.accum)
    _same_bits("frame", bufs["frame"], F.frame)
    for k, b in (("normal", F.normal), ("color", F.color), ("albedo", F.albedo)):
        _same_bits(k, bufs[k], b)
    assert (F.frame != rc.FRAME_SENTINEL).any()


@pytest.fixture(scope="module")
def expected(oracle):
    return {c.name: (c, c.state()) + c.expected(oracle.make_color) for c in rc.cases()}


def test_the_cases_cover_the_shapes(expected):
    names = set(expected)
    sizes = {c.size for c, _, _, _ in expected.values()}
    assert sizes == {(1, 1), (64, 4), (65, 5), (70, 6), (130, 9)}
    assert {c.max_depth for c, _, _, _ in expected.values()} == {1, 4, 8}
    spps = set()
    for c, st, bufs, last in expected.values():
        spps |= {P.spp for P in c.passes()[0]}
    assert spps >= {1, 2, 5, 32}
    assert len(names) == len(rc.cases())


@pytest.mark.parametrize("case", rc.cases(), ids=lambda c: c.name)
def test_a_case_reaches_what_it_is_for(expected, case):
    c, st, bufs, last = expected[case.name]
    w, h = c.size
    before = c.prefill()
    passes, slots, launches = c.passes()
    written = last >= 0
    own = bufs["frame"] != 0
    # every slot state and every alpha flag occurs among the live slots; cells beyond the counted segments are NaN
    live = st["state"] != rc.DEAD_STATE
    if slots >= 64:
        depth = (st["state"][live] >> 8).astype(int)
        assert {0, c.max_depth, c.max_depth + 5} <= set(depth.tolist()) and (c.max_depth == 1 or ((depth > 0) & (depth < c.max_depth)).any())
        for f in (0, rr.ALPHA_ONE, rr.ALPHA_SET, rr.ALPHA_ONE | rr.ALPHA_SET):
            assert ((st["state"][live] & 12) == f).any()
        assert np.isnan(st["cells"][live]).any()
    # what is written is finite although the state holds NaN where nothing may read
    assert np.isfinite(bufs["accum"][written]).all()
    # untouched pixels keep what they held
    keep = ~written if not (c.render is not None and c.world > 1 and c.rank != 0) else np.zeros_like(written)
    assert np.array_equal(bufs["accum"][keep].view(np.uint32), before["accum"][keep].view(np.uint32))
    assert (bufs["frame"][keep] == rc.FRAME_SENTINEL).all()
    n = c.name
    if "_fov" in n:
        assert set(np.unique(last)) == {-1, 0, 1, 2}, np.unique(last)                 # three rings and a gap
    if "uniform" in n:
        assert written.all()
    if "gaze_top_left" in n:
        assert last[0, 0] == 2 and passes[1].offx > 0x80000000
    if "gaze_bottom_right" in n:
        assert last[h - 1, w - 1] == 2
    if "straddle" in n:
        assert written[2:6, 62:66].all() and not written[:2].any()                       # a block over x = 63 | 64 and y = 3 | 4
    if "from_column_0" in n:
        assert written[0, :128].all() and not written[:, 128:].any()
    if "beyond_the_frame" in n:
        P = passes[0]
        assert (P.gw - 1) * P.fx + P.offx >= w and (P.gh - 1) * P.fy + P.offy >= h and written[h - 1, w - 1]
    if "wrapped_offset" in n:
        assert passes[0].offx > 0x80000000 and written[0, 0] and written[h - 1, w - 1] and not written.all()
    if "overlapping" in n:
        assert passes[0].fill > passes[0].fx
    if "ring_launch" in n:
        assert not written[c.gaze[1], c.gaze[0]] and written.any() and not written.all()
    if "accumulate" in n:
        # a blend happened exactly where the reference blends, and the history holds values above 10 and below 0
        blends = c.accumulate and c.subframe > 0 and not (c.launch or {}).get("redraw", 0)
        assert (before["accum"] > 10).any() and (before["accum"] < 0).any()
        plain = rc.Case(n, c.size, gaze=c.gaze, render=c.render, launch=c.launch, max_depth=c.max_depth, accumulate=0, subframe=0, seed=c.seed)
        pb, _ = plain.expected(lambda rgb: np.zeros(len(rgb), np.uint32), st)
        differs = (pb["accum"].view(np.uint32) != bufs["accum"].view(np.uint32)).any(axis=-1)
        assert differs.any() == bool(blends), (blends, int(differs.sum()))
        if blends:
            assert (pb["accum"][written][:, :3] > 10).any()                               # the clamp at 10 is reached
    if c.world > 1:
        zeroed = written & (bufs["frame"] == 0)
        assert zeroed.any() and (written & own).any()
        assert (bufs["accum"][zeroed] == 0).all()
        if c.render is not None and c.rank != 0:
            assert (bufs["frame"][~written] == 0).all()
        else:
            assert (bufs["frame"][~written] == rc.FRAME_SENTINEL).all()
    if c.guides:
        assert (bufs["normal"][written & own][:, 3] == 1).all() and (bufs["normal"][~(written & own)] == rc.GUIDE_SENTINEL).all()
    else:
        assert (bufs["normal"] == rc.GUIDE_SENTINEL).all()
