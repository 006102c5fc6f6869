"""What the gather-plan tests on the CPU and on the GPU share: the frames, and the restated plan of each, computed once.

Every case is the smallest frame found that reaches what it is for; `reaches` holds the properties it exists for, which
tests/test_gather_plan_cpu.py measures again on the restated owner map (gather_ref.shape_of) -- nothing is taken on trust.

    blocks           blocks of 256 pixels: k_plan_owner / k_plan_fill's grid, the block counts k_plan_scan scans
    per              block counts per thread of k_plan_scan, ceil(blocks / 1024)
    scan_last        (the last thread of k_plan_scan that has a chunk, the blocks in that chunk)
    last_block       pixels in the last block
    holes            pixels nobody writes
    empty_ranks      ranks that own nothing (pack does not launch at all)
    owners_per_wave  (min, max) distinct owners among 64 consecutive pixels: the turns of k_plan_fill's ballot loop
    counts           (min, max) of the ranks' counts
    words_above      max(counts) (pack) or the plan's total (unpack) lies above 2048 * 256 words: the grid-stride loop turns"""
import collections

import numpy as np

import gather_ref as gr

Case = collections.namedtuple("Case", "name size gaze radii uniform world tile reaches")
LOOP_WORDS = gr.MOVE_GRID * gr.MOVE_BLOCK          # 524 288: above it k_gather_pack / k_gather_unpack's loop turns


def _c(name, size, gaze, radii, world, tile=None, **reaches):
    return Case(name, size, gaze if gaze is not None else (size[0] // 2, size[1] // 2), radii, radii is None, world, tile, reaches)


CASES = [
    _c("one_pixel", (1, 1), None, None, 1, blocks=1, last_block=1, holes=0, counts=(1, 1)),
    _c("no_periphery", (3, 2), (1, 1), (1, 4), 2, periphery_grid=(0, 0), passes_seen=[2], exact_counts=[6, 0], empty_ranks=1, holes=0),
    _c("no_periphery_last_rank", (3, 2), (1, 1), (1, 4), 3, periphery_grid=(0, 0), passes_seen=[2], exact_counts=[0, 0, 6], empty_ranks=2),
    _c("holes", (70, 6), None, (1, 4), 3, holes=130, passes_seen=[0, 1, 2], blocks=2, last_block=164, empty_ranks=0),
    _c("owners64", (256, 1), None, None, 64, (1, 1), owners_per_wave=(64, 64), counts=(4, 4), blocks=1),
    _c("owners63_ragged", (257, 3), None, None, 63, (1, 1), owners_per_wave=(3, 63), full_wave_owners=(62, 63), blocks=4, last_block=3, counts=(12, 14)),
    _c("todays_frame", (200, 120), (150, 40), (14, 44), 8, blocks=94, per=1, passes_seen=[0, 1, 2]),
    _c("chunked_scan", (640, 410), (639, 0), (24, 80), 7, blocks=1025, per=2, scan_last=(512, 1), holes=1280),
    _c("long_pack", (1024, 513), None, None, 1, blocks=2052, per=3, scan_last=(683, 3), pack_words_above=LOOP_WORDS, counts=(525312, 525312)),
    _c("long_unpack", (1024, 513), None, None, 5, (16, 16), blocks=2052, per=3, unpack_words_above=LOOP_WORDS, empty_ranks=0),
    _c("many_ranks_odd_tiles", (1024, 513), (700, 200), (60, 200), 64, (5, 3), blocks=2052, per=3, max_owners_per_wave=14, empty_ranks=0,
       passes_seen=[0, 1, 2]),
    _c("gaze_outside", (130, 9), (5000, 7000), (2, 5), 2, passes_seen=[0, 2], fovea_only_on_last_row_and_column=True),
    _c("one_tile", (65, 5), None, None, 4, (128, 64), exact_counts=[325, 0, 0, 0], empty_ranks=3),
    _c("one_tile_per_pass", (130, 40), (60, 20), (3, 8), 4, (128, 64), owner_is_pass=True, empty_ranks=1, passes_seen=[0, 1, 2]),
    _c("default_tiles", (70, 6), None, (1, 4), 3, (0, -1), same_plan_as="holes"),
]
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]
SMALL = [c for c in CASES if c.size[0] * c.size[1] <= 200 * 120]          # cheap enough for the painting restatements of other modules

_memo = {}


def restated(case):
    """-> (owner map (h, w) uint8, per rank the ascending pixel indices, counts) of a case, computed once and read-only."""
    key = case[:7] if isinstance(case, Case) else tuple(case)
    if key not in _memo:
        _, size, gaze, radii, uniform, world, tile = key
        owner = gr.owner_map(size, gaze, radii, uniform, world, tile)
        lists, counts = gr.plan_of(owner, world)
        owner.setflags(write=False)
        for a in lists:
            a.setflags(write=False)
        _memo[key] = (owner, lists, counts)
    return _memo[key]


def restated_for(size, gaze, radii, uniform, world, tile):
    """The same for parameters that are no named case (the cache test's variations)."""
    return restated(("", tuple(size), tuple(gaze), tuple(radii) if radii is not None else None, bool(uniform), int(world),
                     tuple(tile) if tile is not None else None))


def random_words(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
