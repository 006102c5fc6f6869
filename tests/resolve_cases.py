"""The frames and path states of the resolve tests (tests/test_resolve_state_cpu.py, tests/test_resolve_state_gpu.py): for
every case the launch parameters and configuration, a path state in slot order made from a seed, the frame buffers as they are
before the resolve, and -- through tests/resolve_ref.py -- what the resolve must leave in them.

The frames are the smallest that reach what a case is for: k_resolve works in 64 x 4 pixel tiles, so 1 x 1, 64 x 4 (one full
tile), 65 x 5 (one pixel into the next tiles), 70 x 6 and 130 x 9 (three tile columns and rows, the last ones partial).

A path state holds what nothing may read as NaN or as a pattern: the cells beyond a slot's counted segments, alpha[slot]
without ALPHA_SET, and everything of the launch indices that fail the ring test (their state word is 0xffffffff)."""
import numpy as np

import resolve_ref as rr
from fovpathtracing_optixcodelatest_amd import abi

FRAME_SENTINEL = 0x01020304
GUIDE_SENTINEL = np.float32(7.25)
DEAD_STATE = 0xffffffff


class Case:
    def __init__(self, name, size, gaze=None, render=None, launch=None, max_depth=4, accumulate=0, subframe=0, guides=0, world=1, rank=0,
                 seed=1):
        """render: dict(uniform spp) or dict(radii=(r_inner, r_outer), spp=(P, M, F)); launch: dict(grid, factor, fill, offset,
        r_inner, r_outer, spp, redraw)."""
        assert (render is None) != (launch is None)
        self.name, self.size, self.render, self.launch = name, size, render, launch
        self.gaze = gaze if gaze is not None else (size[0] // 2, size[1] // 2)
        self.max_depth, self.accumulate, self.subframe, self.guides, self.world, self.rank, self.seed = max_depth, accumulate, subframe, guides, world, rank, seed

    def __repr__(self):
        return self.name

    # -- the parameters, on a renderer's (or a bare) abi.LaunchParams -----------------------------------
    def config(self):
        c = abi.Config.reference_default()
        c.max_depth, c.accumulate, c.write_guides, c.world, c.rank = self.max_depth, self.accumulate, self.guides, self.world, self.rank
        if self.render is not None:
            if "uniform" in self.render:
                c.uniform, c.spp_uniform = 1, self.render["uniform"]
            else:
                c.r_inner, c.r_outer = self.render["radii"]
                c.spp_periphery, c.spp_middle, c.spp_fovea = self.render["spp"]
        return c

    def set_params(self, lp):
        f = lp.frame
        f.size.x, f.size.y = self.size
        f.c.x, f.c.y = self.gaze
        f.subframe_index = self.subframe
        if self.launch is not None:
            L = self.launch
            f.factor.x, f.factor.y, f.factor.z = L["factor"], L["factor"], 1
            f.fillSize = L["fill"]
            f.offset.x, f.offset.y = L["offset"][0] & 0xffffffff, L["offset"][1] & 0xffffffff
            f.r_inner, f.r_outer = L.get("r_inner", 0.0), L.get("r_outer", 1e9)
            f.redraw = L.get("redraw", 0)
            lp.samples_per_launch = L["spp"]

    def grid(self):
        return self.launch["grid"] if self.launch is not None else (0, 0)

    def passes(self):
        """The passes after resolve_ref, placed in the arrays -> (passes, sample slots, launch records)."""
        lp = abi.LaunchParams()
        self.set_params(lp)
        ps = rr.launch_pass(lp, *self.grid()) if self.launch is not None else rr.render_passes(self.config(), lp)
        slots, launches = rr.layout(ps)
        return ps, slots, launches

    # -- the path state ------------------------------------------------------------------------------------
    def state(self):
        """-> dict(state, cells, alpha, backplate, guide_n, guide_a) in slot order."""
        ps, slots, launches = self.passes()
        g = np.random.default_rng(self.seed)
        D = self.max_depth
        depths = np.array(sorted({0, 1, (D + 1) // 2, D, D + 1, D + 5}))
        depth = g.choice(depths, slots)
        flags = g.choice([0, rr.ALPHA_ONE, rr.ALPHA_SET, rr.ALPHA_ONE | rr.ALPHA_SET], slots) | g.integers(0, 4, slots)   # (DONE, SECONDARY: not the resolve's business)
        state = (flags | (depth << 8)).astype(np.uint32)
        cells = g.random((slots, D, 4), np.float32) * np.float32(3.0)
        cells[g.random(slots) < 0.1] *= np.float32(20.0)                    # means above the accumulate clamp of 10
        cells[g.random(slots) < 0.1] = 0.0
        cells[np.arange(D)[None, :] >= np.minimum(depth, D)[:, None]] = np.nan          # beyond the counted segments: not to be read
        alpha = g.random((slots, 4), np.float32) * np.float32(1.5)
        alpha[(flags & rr.ALPHA_SET) == 0] = np.nan
        backplate = g.random((launches, 4), np.float32) * np.float32(2.0)
        guide_n = g.random((slots, 4), np.float32) * np.float32(2.0) - np.float32(1.0)
        guide_a = g.random((slots, 4), np.float32)
        for p, P in enumerate(ps):                                           # the launch indices that fail the ring test
            for li in range(P.gw * P.gh):
                if not P.alive(li % P.gw, li // P.gw, self.gaze):
                    s0 = P.slot_base + li * P.spp
                    state[s0:s0 + P.spp] = DEAD_STATE
                    cells[s0:s0 + P.spp] = np.nan
                    alpha[s0:s0 + P.spp] = np.nan
                    guide_n[s0:s0 + P.spp] = np.nan
                    guide_a[s0:s0 + P.spp] = np.nan
                    backplate[P.launch_base + li] = np.nan
        return dict(state=state, cells=cells, alpha=alpha, backplate=backplate, guide_n=guide_n, guide_a=guide_a)

    def prefill(self):
        """The frame buffers before the resolve: a history with values above 10 and below 0, patterns elsewhere."""
        w, h = self.size
        g = np.random.default_rng(self.seed + 1000)
        accum = (g.random((h, w, 4), np.float32) * np.float32(16.0) - np.float32(2.0)).astype(np.float32)
        return dict(accum=accum, frame=np.full((h, w), FRAME_SENTINEL, np.uint32),
                    normal=np.full((h, w, 4), GUIDE_SENTINEL, np.float32), color=np.full((h, w, 4), GUIDE_SENTINEL, np.float32),
                    albedo=np.full((h, w, 4), GUIDE_SENTINEL, np.float32))

    def expected(self, make_color, st=None):
        """-> (frame buffers after the resolve, map of the last writing pass)."""
        ps, slots, launches = self.passes()
        st = st if st is not None else self.state()
        bufs = self.prefill()
        last = rr.resolve(ps, self.gaze, self.max_depth, self.accumulate, st["state"], st["cells"], st["alpha"], st["backplate"], bufs, make_color,
                          guide_n=st["guide_n"] if self.guides else None, guide_a=st["guide_a"] if self.guides else None,
                          rank=self.rank, world=self.world, whole_frame=self.render is not None)
        return bufs, last


def _fov(radii, spp):
    return dict(radii=radii, spp=spp)


def _block(grid, factor, fill, offset, spp, **kw):
    return dict(grid=grid, factor=factor, fill=fill, offset=offset, spp=spp, **kw)


def cases():
    c = [
        # uniform launches: every tile shape, spp and depth cap
        Case("1x1_uniform_depth1", (1, 1), render=dict(uniform=1), max_depth=1),
        Case("64x4_uniform_spp2", (64, 4), render=dict(uniform=2)),
        Case("65x5_uniform_spp5_guides", (65, 5), render=dict(uniform=5), guides=1),
        Case("70x6_uniform_depth8", (70, 6), render=dict(uniform=1), max_depth=8),
        # the three passes of render(): all three rings and pixels nobody writes (columns / rows beyond the last 4 x 4 block)
        Case("70x6_fov", (70, 6), render=_fov((1, 4), (1, 2, 5))),
        Case("70x6_fov_guides", (70, 6), render=_fov((1, 4), (2, 1, 2)), guides=1, seed=2),
        Case("130x9_fov_spp32_depth8", (130, 9), render=_fov((2, 3), (1, 2, 32)), max_depth=8),
        Case("130x9_fov_gaze_top_left", (130, 9), gaze=(0, 0), render=_fov((2, 5), (1, 2, 2))),
        Case("130x9_fov_gaze_bottom_right", (130, 9), gaze=(129, 8), render=_fov((2, 5), (2, 1, 2)), max_depth=1),
        Case("130x9_fov_accumulate_sub3", (130, 9), render=_fov((2, 5), (1, 2, 2)), accumulate=1, subframe=3),
        # single launches: 4 x 4 blocks across a 64-column and a 4-row tile edge, beyond the frame (clamped), overlapping
        Case("130x9_blocks_straddle_tiles", (130, 9), launch=_block((6, 2), 4, 4, (54, 2), 2)),
        Case("130x9_blocks_from_column_0", (130, 9), launch=_block((32, 2), 4, 4, (0, 0), 1)),
        Case("70x6_grid_beyond_the_frame", (70, 6), launch=_block((6, 3), 4, 4, (58, 0), 2)),
        # (launch indices at wrapped pixel indices pass the ring test only when the gaze is such an index; they are clamped onto the last column / row)
        Case("70x6_wrapped_offset", (70, 6), gaze=(0xfffffffc, 0xfffffffe), launch=_block((5, 3), 2, 2, (-4, -2), 1, r_outer=1e10)),
        Case("65x5_overlapping_fills", (65, 5), launch=_block((30, 2), 2, 4, (1, 0), 2)),
        Case("65x5_overlapping_fills_accumulate_sub3", (65, 5), launch=_block((30, 2), 2, 4, (1, 0), 2), accumulate=1, subframe=3),
        Case("65x5_ring_launch", (65, 5), gaze=(30, 2), launch=_block((65, 5), 1, 1, (0, 0), 2, r_inner=2.0, r_outer=20.0)),
        # accumulate mode
        Case("65x5_accumulate_off_sub3", (65, 5), launch=_block((65, 5), 1, 1, (0, 0), 2), accumulate=0, subframe=3),
        Case("65x5_accumulate_sub0", (65, 5), launch=_block((65, 5), 1, 1, (0, 0), 2), accumulate=1, subframe=0),
        Case("65x5_accumulate_sub3", (65, 5), launch=_block((65, 5), 1, 1, (0, 0), 2), accumulate=1, subframe=3),
        Case("65x5_accumulate_sub3_redraw", (65, 5), launch=_block((65, 5), 1, 1, (0, 0), 2, redraw=1), accumulate=1, subframe=3),
        # a frame sharded over two ranks
        Case("130x9_fov_world2_rank0", (130, 9), render=_fov((2, 5), (1, 2, 2)), world=2, rank=0),
        Case("130x9_fov_world2_rank1", (130, 9), render=_fov((2, 5), (1, 2, 2)), world=2, rank=1),
        Case("130x9_launch_world2_rank1", (130, 9), launch=_block((20, 2), 4, 4, (10, 0), 1), world=2, rank=1),
        Case("130x9_uniform_world2_rank1_guides", (130, 9), render=dict(uniform=1), world=2, rank=1, guides=1),
    ]
    assert len({k.name for k in c}) == len(c)
    return c
