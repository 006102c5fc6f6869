"""Queue states for the ray-level tests of k_traverse's QUEUE side (fovpt_debug_trace_queued), shared by
tests/test_trace_queue_cpu.py (what the cases reach, no GPU) and tests/test_trace_queue_gpu.py (the library against the oracle).

A case is a scene, a row of LAYOUTS for each of the two queues, and a launch (iterations, grids).  The rays are a seeded choice
of the scene's tests/trace_cases.py batch (mixed(tri, 7)), so one oracle run per scene serves every case.  Nothing here restates
an index formula of the library: a layout is counts per shard, and the place of ray i follows from the counts alone -- the
rays fill the shards in order (places())."""
import numpy as np

import trace_cases as tc
from fovpathtracing_optixcodelatest_amd import abi

MAX_DEPTH = 3
ALPHA = abi.DEBUG_TRACE_ALPHA
TARGETS = (0, 1, 2, ALPHA)
RAY_SEED = 7
SEED0 = 5980                                # the first base seed from 100 up under which every ray set but the one ray of `last_one` meets the
                                            # oracle-only conditions of tests/test_trace_queue_cpu.py on both scenes (shares and targets)
SCENES = {"cornell": tc.cornell, "soup256": lambda: tc.soup(256, 3)}
DECOY = (7, 3, 11, 0, 5, 2, 9, 1)          # counts no row below has: a launch that reads a neighbouring counter word sees another queue

# name -> (sel, the counts of the launch's rays per shard, the counts of the other chain's rays, slots: 0 = 8 * n).
# `brim`: a state of 8 sample slots has shards of 8 / 8 + 512 = 513 entries, which three of its shards fill to the last one.
LAYOUTS = {
    "one_shard_0": (0, (40, 0, 0, 0, 0, 0, 0, 0), None, 0),
    "one_shard_3": (0, (0, 0, 0, 40, 0, 0, 0, 0), None, 0),
    "one_shard_7": (0, (0, 0, 0, 0, 0, 0, 0, 40), None, 0),
    "even": (0, (25,) * 8, None, 0),
    "slivers": (0, (3, 1, 0, 2, 1, 0, 0, 5), None, 0),
    "aligned": (0, (16, 32, 0, 16, 48, 16, 0, 16), None, 0),
    "empty_ends": (0, (0, 0, 37, 0, 0, 41, 0, 0), None, 0),
    "last_one": (0, (0, 0, 0, 0, 0, 0, 0, 1), None, 0),
    "uneven": (0, (1, 15, 17, 31, 33, 63, 65, 7), None, 0),
    "brim": (0, (513, 1, 0, 513, 0, 0, 2, 513), None, 8),
    "chain1": (1, (17, 0, 5, 30, 0, 0, 0, 0), (0, 0, 0, 0, 9, 9, 9, 9), 0),
    "chain2": (2, (0, 0, 0, 0, 0, 21, 1, 30), (9, 9, 9, 9, 0, 0, 0, 0), 0),
}


def partner(name):
    """The counts of the OTHER queue of a case whose one queue has the row `name`: both queues hold the same n rays, so the other
    one needs a row of the same sum that puts every shard boundary elsewhere.  For a one-shard row that is the next one-shard row;
    for `even`, whose mirror image is itself, the 200 rays cut at 15, 65, 115 and 165 -- under one unit of 256 threads the four
    occlusion waves own the pools [0, 50), [50, 100), ..., a wave's first refill takes 16 rays, and the 16th is then the first
    entry of the next shard: the one index at which `<` and `<=` in phys16's fast path differ; for
    `last_one`, whose mirror image would put its ray at entry 0 of shard 0 (slot 0, place 0), the one ray in shard 3; for every
    other row its mirror image inside the selection."""
    sel, counts, _, _ = LAYOUTS[name]
    if name.startswith("one_shard_"):
        return LAYOUTS["one_shard_%d" % {0: 3, 3: 7, 7: 0}[int(name[-1])]][1]
    if name == "even":
        return (15, 50, 0, 50, 50, 0, 35, 0)
    if name == "last_one":
        return (0, 0, 0, 1, 0, 0, 0, 0)
    if sel == 0:
        return counts[::-1]
    return counts[:4][::-1] + counts[4:][::-1]


ITERS = ((0, 0), (1, 3), (62, 62), (5, 4))       # (it_closest, it_shadow)
GRIDS_CLOSEST = (1, 2, 0)                       # units of 256 threads: 4 and 8 one-wave blocks, and what a job uses
GRIDS_SHADOW = (1, 0)


class Run:
    """One launch: the radiance queue has the row `layout` and the shadow queue its partner, or (swap) the other way round."""

    def __init__(self, layout, swap, iters, grid_closest, grid_shadow):
        self.layout, self.swap, self.iters, self.grid_closest, self.grid_shadow = layout, swap, iters, grid_closest, grid_shadow
        self.sel, row, self.other_counts, self.slots = LAYOUTS[layout]
        self.q_count, self.sq_count = (partner(layout), row) if swap else (row, partner(layout))
        self.n = sum(row)
        self.n_other = sum(self.other_counts) if self.other_counts else 0
        self.name = "%s%s-it%d.%d-g%d.%d" % (layout, "~" if swap else "", iters[0], iters[1], grid_closest, grid_shadow)


def runs():
    """A thin product: every row as the radiance queue and as the shadow queue, the iterations and the grids cycling (every pair
    of grids and every pair of iterations occurs); then the 200 rays of `even` under all six pairs of grids, and each chain
    under one unit for either launch: rounds and pools of several rays inside four shards."""
    out, k = [], 0
    for name in LAYOUTS:
        for swap in (False, True):
            out.append(Run(name, swap, ITERS[k % 4], GRIDS_CLOSEST[k % 3], GRIDS_SHADOW[(k // 3) % 2]))
            k += 1
    out += [Run("even", False, ITERS[1], gc, gs) for gc in GRIDS_CLOSEST for gs in GRIDS_SHADOW]
    out += [Run("chain1", False, ITERS[3], 1, 1), Run("chain2", True, ITERS[1], 1, 1)]
    assert len({r.name for r in out}) == len(out)
    return out


_batches = {}


def batch(scene):
    """(triangles, origins, dirs) of a scene: all rays of its tests/trace_cases.py batch."""
    if scene not in _batches:
        tri = SCENES[scene]()
        o, d, _ = tc.mixed(tri, RAY_SEED)
        _batches[scene] = (tri, o, d)
    return _batches[scene]


def _slots(rng, n, first):
    """A seeded shuffle composed with a reversal; a ray whose slot would be its own index trades with its neighbour."""
    slot = (n - 1 - rng.permutation(n)).astype(np.int64)
    for i in range(n):
        if slot[i] == i and n > 1:
            j = (i + 1) % n
            slot[i], slot[j] = slot[j], slot[i]
    return (slot + first).astype(np.uint32)


def _records(index):
    """vis4 and occ4 of the rays with these running numbers: distinct per ray in all four components, exact in binary32."""
    i = np.asarray(index, np.float64)[:, None]
    k = np.arange(4, dtype=np.float64)[None, :]
    return (4096.0 * (k + 1) + i + 0.25).astype(np.float32), (-(4096.0 * (k + 1) + i) - 0.5).astype(np.float32)


def rays_of(scene, layout):
    """The ray sets of a layout on a scene -> (mine, other or None): dict(pick = indices into batch(scene), o, d, slot, target,
    vis, occ).  The same for every launch of the layout; the other chain's rays are disjoint from the launch's own."""
    _, o, d = batch(scene)
    sel, counts, other_counts, _ = LAYOUTS[layout]
    n, m = sum(counts), sum(other_counts) if other_counts else 0
    rng = np.random.default_rng(SEED0 + list(LAYOUTS).index(layout))
    total = len(o)
    pick = rng.permutation(total)
    if n + m > total:                                   # (brim: two rays more than the batch has -- two of them twice)
        pick = np.concatenate([pick, rng.choice(total, n + m - total, replace=False)])

    def make(idx, first):
        k = len(idx)
        vis, occ = _records(first + np.arange(k))
        return dict(pick=idx, o=o[idx], d=d[idx], slot=_slots(rng, k, first), target=np.array(TARGETS, np.uint32)[np.arange(k) % 4], vis=vis, occ=occ)

    return make(pick[:n], 0), (make(pick[n:n + m], n) if m else None)


def places(counts):
    """Where the rays lie that fill the shards in order: (shard, entry) per ray -- from the counts alone."""
    shard = np.repeat(np.arange(8), counts)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return shard, np.arange(len(shard)) - first[shard]
