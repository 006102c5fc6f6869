"""What the cases of tests/trace_queue_cases.py reach, shown without a GPU: the oracle alone says that their rays hit and miss,
are occluded and are not, under every target; and a Python walk of the index arithmetic of a traversal launch (ShardMap::load,
phys and phys16 of csrc/fovpt_queue.h; the grid-stride loop, the block clamp, the pool partition and the refill of
csrc/traverse.hip) says which branches of it the launches take -- and that a mutant of each would put a ray elsewhere on at
least one case.  The walk shows reach only: no GPU test takes an expected value from it, and no mutated kernel is ever run on
a GPU, where a wrong index can leave the buffers."""
import numpy as np
import pytest

import trace_cases as tc
import trace_queue_cases as qc

MISS = 0xFFFFFFFF
NUM_CUS = 256                       # of the device the production grids are worked out for (an MI355X)
# The launch constants the walk uses, by the names the sources define them under (test_the_walk_has_the_sources_constants
# reads the defines and holds these to them)
DEFINES = {"FOVPT_BLOCK": 256, "FOVPT_TBLOCK": 64, "FOVPT_GRID_PER_CU": 24, "FOVPT_GRID_SHADOW_PER_CU": 6, "FOVPT_MAX_ITERS": 63,
           "FOVPT_SHARDS": 8, "FOVPT_SHARD_STRIDE": 128, "FOVPT_REFILL": 6}
BLOCK, TBLOCK, SHARDS = DEFINES["FOVPT_BLOCK"], DEFINES["FOVPT_TBLOCK"], DEFINES["FOVPT_SHARDS"]
TQUADS, REFILL = TBLOCK // 4, DEFINES["FOVPT_REFILL"]                          # rays per wave and round; idle quads that trigger a refill
STRIDE, MAX_ITERS = DEFINES["FOVPT_SHARD_STRIDE"], DEFINES["FOVPT_MAX_ITERS"]  # counter words per shard; iterations
CAP_SLACK = 512                     # shard_capacity(slots) = slots / FOVPT_SHARDS + 512 (csrc/fovpt_jobplan.h)


def _capacity(run):
    return (run.slots or SHARDS * max(run.n, 1)) // SHARDS + CAP_SLACK


def test_the_walk_has_the_sources_constants():
    """The defines of csrc/fovpt_device.h, csrc/fovpt_jobplan.h and csrc/traverse.hip, the capacity rule of csrc/fovpt_jobplan.h and
    the grids per CU that csrc/fovpt_api.hip gives the traversal launches are what the walk
    assumes: a change of the block size, the refill threshold, the grids per CU or the counter layout fails here, not silently in
    the reach shown below.  One wave per block, eight shards and two chains of four are built into the walk's shape."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fovpathtracing_optixcodelatest_amd", "csrc")
    text = "".join(open(os.path.join(csrc, f)).read() for f in ("fovpt_device.h", "fovpt_jobplan.h", "traverse.hip"))
    for name, value in DEFINES.items():
        found = re.findall(r"^\s*#define\s+%s\s+(\d+)\b" % name, text, flags=re.M)
        assert found and all(int(x) == value for x in found), (name, found, value)
    assert TBLOCK == 64 and SHARDS == 8
    assert re.search(r"#define\s+FOVPT_TQUADS\s+\(FOVPT_TBLOCK\s*/\s*4\)", text)
    assert re.search(r"#define\s+FOVPT_CNT_SQ\(it\)\s+\(FOVPT_MAX_ITERS \+ 1 \+ \(it\)\)", text) and re.search(r"#define\s+FOVPT_CNT_Q\(it\)\s+\(it\)", text)
    assert "return (uint32_t)(slots / FOVPT_SHARDS + %d);" % CAP_SLACK in text
    api = open(os.path.join(csrc, "fovpt_api.hip")).read()
    assert '{"FOVPT_GRID", 64, FOVPT_GRID_PER_CU, &E.grid_trace}' in api and '{"FOVPT_GRID_SHADOW", 16, FOVPT_GRID_SHADOW_PER_CU, &E.grid_shadow}' in api
    assert "*g.grid = shard_grid(c->num_cus * per_cu);" in api


# ---- the oracle alone: the rays of every case hit and miss, are occluded and are not -----------------------------------------
@pytest.fixture(scope="module")
def truth(oracle):
    out = {}
    for scene in qc.SCENES:
        tri, o, d = qc.batch(scene)
        out[scene] = oracle.OracleScene(tc.model_of(tri)).trace(o, d, brute=True)
    return out


@pytest.mark.parametrize("scene", sorted(qc.SCENES))
def test_batches_have_1540_rays(scene):
    assert len(qc.batch(scene)[1]) == 1540


@pytest.mark.parametrize("scene", sorted(qc.SCENES))
def test_rays_hit_and_miss_and_are_occluded_and_are_not(truth, scene):
    """Conditions on the inputs, not measurements: every ray set of every case -- the launch's own and the other chain's, 12 to
    1542 rays -- holds at least 8 % misses, 8 % hits, 10 % occluded and 10 % unoccluded rays, and every target occurs among its
    occluded and among its unoccluded rays.  The one exception is `last_one`: its single ray is whatever it is.  (The smallest
    shares over the whole batches are misses 10 % (cornell) and 15 % (soup256), unoccluded 16.5 % and 34 %; the base seed of
    the choices, trace_queue_cases.SEED0, was picked by these conditions alone.)"""
    prim, _, occ = truth[scene]
    shares, exempt = {}, []
    for layout in qc.LAYOUTS:
        for rays in qc.rays_of(scene, layout):
            if rays is None:
                continue
            p, oc = prim[rays["pick"]], occ[rays["pick"]].astype(bool)
            n = len(p)
            if layout == "last_one":
                exempt.append((layout, n))
                continue
            miss, occluded = int((p == MISS).sum()), int(oc.sum())
            shares[(layout, n)] = (miss / n, occluded / n)
            assert miss >= 0.08 * n and n - miss >= 0.08 * n, (scene, layout, n, miss)
            assert occluded >= 0.10 * n and n - occluded >= 0.10 * n, (scene, layout, n, occluded)
            for t in qc.TARGETS:
                m = rays["target"] == t
                assert (oc & m).any() and (~oc & m).any(), (scene, layout, "target", t)
    assert exempt == [("last_one", 1)] and len(shares) == len(qc.LAYOUTS) + 1        # (both chains' other sets, less last_one)
    print(scene, {k: "%.3f %.3f" % v for k, v in shares.items()})


def test_slots_targets_and_records():
    """Slots are a permutation in which no ray's slot is its own index; targets cycle through the three cells and alpha; vis4 and
    occ4 are distinct per ray in all four components, and their .w is not the +0 the launch must store; the other chain's rays
    are none of the launch's own."""
    for layout, (sel, counts, other_counts, _) in qc.LAYOUTS.items():
        mine, other = qc.rays_of("cornell", layout)
        n = sum(counts)
        assert sorted(mine["slot"].tolist()) == list(range(n))
        if n > 1:
            assert not (mine["slot"] == np.arange(n)).any(), layout
        assert mine["target"][:4].tolist() == list(qc.TARGETS) or n < 4
        both = [mine] + ([other] if other is not None else [])
        vis, occ = np.concatenate([r["vis"] for r in both]), np.concatenate([r["occ"] for r in both])
        rec = np.concatenate([vis, occ])
        for k in range(4):
            assert len(np.unique(rec[:, k])) == len(rec), (layout, k)
        assert (rec[:, 3] != 0).all()
        if other is not None:
            m = len(other["pick"])
            assert sorted(other["slot"].tolist()) == list(range(n, n + m)) and not np.intersect1d(mine["pick"], other["pick"]).size
        for swap in (False, True):
            r = qc.Run(layout, swap, (0, 0), 0, 0)
            assert sum(r.q_count) == sum(r.sq_count) == n and tuple(r.q_count) != tuple(r.sq_count), layout
            # no ray whose slot is its index AND its place in a queue
            for c in (r.q_count, r.sq_count):
                shard, entry = qc.places(c)
                cap = _capacity(r)
                assert not ((mine["slot"] == np.arange(n)) & (shard * cap + entry == np.arange(n))).any(), (layout, swap)
            assert tuple(qc.DECOY) not in (tuple(r.q_count), tuple(r.sq_count))


# ---- a walk of the launch's index arithmetic ------------------------------------------------------------------------------------
class ShardMap:
    """ShardMap::load, phys and phys16 as csrc/fovpt_queue.h writes them, with a log of the branches taken."""

    def __init__(self, words, word, sel, cap, mutant, log):
        f = 4 if sel == 2 else 0
        self.cap, self.mutant, self.log = cap, mutant, log
        self.first_cap = 0 if mutant == "first_cap dropped" else f * cap
        p = [0]
        for k in range(4):
            p.append(p[-1] + words[f + k][word])
        if sel == 0 or mutant == "p5..p8 not collapsed":
            for k in range(4, 8):
                p.append(p[-1] + words[k][word])
        else:
            p += [p[4]] * 4
        self.p = p
        if self.first_cap:
            log.add("first_cap != 0")

    def total(self):
        return self.p[8]

    def _shard(self, i):
        s = 0
        for k in range(1, 8):
            if i >= self.p[k]:
                s = k
        return s

    def phys(self, i):
        s = self._shard(i)
        if any(self.p[k] == self.p[k + 1] for k in range(s)):
            self.log.add("empty shard skipped")
        self.log.add("s = %d" % s)
        return self.first_cap + s * self.cap + (i - self.p[s])

    def phys16(self, i, i0):
        s = self._shard(i0)
        nxt = self.p[s + 1] if s < 7 else 0xFFFFFFFF
        fast = i0 + 15 <= nxt if self.mutant == "<= for < in the fast path" else i0 + 15 < nxt
        if fast:
            self.log.add("fast path")
            self.log.add("s = %d" % s)
            return self.first_cap + s * self.cap - self.p[s] + i
        self.log.add("fallback")
        return self.phys(i)


def _blocks(grid, cap, sel, shadow, log):
    """fovpt_launch_traverse: one-wave blocks of a grid given in units of 256 threads, and the clamp of a closest-hit launch."""
    blocks = max(grid * BLOCK // TBLOCK, 1)
    if not shadow:
        rounds = ((4 if sel else 8) * cap + TQUADS - 1) // TQUADS
        if blocks > rounds:
            blocks = (rounds + SHARDS - 1) // SHARDS * SHARDS
            log.add("clamped grid")
        else:
            log.add("unclamped grid")
    return blocks


def _duration(idx):
    """Steps an occlusion ray takes in the walk: any fixed function of the ray will do, as long as quads end at different times."""
    return 1 + (idx * 2654435761 >> 7) % 9


def walk(run, mutant=None, log=None):
    """The places a launch of this run visits -> (closest: the place of ray i per i; shadow: sorted (i, place) pairs)."""
    log = set() if log is None else log
    n_all = [a + b for a, b in zip(run.q_count, run.other_counts or (0,) * 8)], [a + b for a, b in zip(run.sq_count, run.other_counts or (0,) * 8)]
    cap = _capacity(run)
    words = [[0] * STRIDE for _ in range(8)]
    itc, its = run.iters
    for s in range(8):
        for w in (itc - 1, itc + 1, its):
            if 0 <= w <= MAX_ITERS:
                words[s][w] = qc.DECOY[s]
        for w in (its - 1, its + 1, itc):
            if 0 <= w <= MAX_ITERS:
                words[s][MAX_ITERS + 1 + w] = qc.DECOY[s]
        words[s][itc] = n_all[0][s]
        words[s][MAX_ITERS + 1 + its] = n_all[1][s]
    off = 1 if mutant == "counter word off by one" else 0
    div = 2 if run.sel else 1
    # closest hit: a static grid-stride over quads, 16 consecutive rays per wave and round
    m = ShardMap(words, itc + off, run.sel, cap, mutant, log)
    blocks = _blocks(run.grid_closest or NUM_CUS * DEFINES["FOVPT_GRID_PER_CU"] // div, cap, run.sel, False, log)
    closest = {}
    for b in range(blocks):
        for lane in range(TQUADS):
            i = b * TQUADS + lane
            while i < m.total():
                closest[i] = m.phys16(i, i - lane)
                i += blocks * TQUADS
    for i0 in range(0, m.total(), TQUADS):
        if len({closest[i] // cap for i in range(i0, min(i0 + TQUADS, m.total()))}) >= 3:
            log.add("a 16-group over 3 shards")
    # occlusion: every wave owns one contiguous pool and refills its idle quads from it
    m = ShardMap(words, MAX_ITERS + 1 + its + off, run.sel, cap, mutant, log)
    nwaves = _blocks(run.grid_shadow or (NUM_CUS * DEFINES["FOVPT_GRID_SHADOW_PER_CU"] + SHARDS - 1) // SHARDS * SHARDS // div, cap, run.sel, True, log)
    n = m.total()
    shadow = []
    per = (n + nwaves - 1) // nwaves if n else 0
    for wave in range(nwaves if n else 0):
        first = min(n, wave * per)
        end = min(n, first + per)
        if mutant == "pool partition unclamped":
            first, end = wave * per, wave * per + per
        if mutant == "wave * per unclamped, alone":
            first = wave * per
        if first >= end:
            log.add("empty pool")
        elif 0 < first < n:
            log.add("pool boundary on a shard boundary" if first in m.p[1:8] else "pool boundary inside a shard")
        left = [0] * TQUADS                      # steps each quad's ray still has to go; 0 = idle
        nxt = first
        while True:
            idle = [q for q in range(TQUADS) if left[q] == 0]
            if len(idle) == TQUADS or (len(idle) >= REFILL and nxt < end):
                for rank, q in enumerate(idle):
                    idx = nxt + rank
                    if idx < end:
                        shadow.append((idx, m.phys16(idx, nxt)))
                        left[q] = _duration(idx)
                if len(idle) < TQUADS:
                    log.add("refill of a running wave")
                nxt = min(end, nxt + (TQUADS if mutant == "next + 16 for next + n_idle" else len(idle)))
                if len(idle) == TQUADS and not any(left):
                    break
            left = [max(x - 1, 0) for x in left]
    return [closest[i] for i in sorted(closest)], sorted(shadow)


def _expected(run, counts):
    """The places the launch's own rays lie at, from the counts alone."""
    cap = _capacity(run)
    shard, entry = qc.places(counts)
    return (shard * cap + entry).tolist()


def test_the_walk_visits_every_ray_once_where_the_counts_put_it():
    for run in qc.runs():
        closest, shadow = walk(run)
        assert closest == _expected(run, run.q_count), run.name
        assert [p for _, p in shadow] == _expected(run, run.sq_count) and [i for i, _ in shadow] == list(range(run.n)), run.name


REACH = ["fast path", "fallback"] + ["s = %d" % s for s in range(8)] + [
    "a 16-group over 3 shards", "empty shard skipped", "first_cap != 0", "pool boundary inside a shard", "pool boundary on a shard boundary",
    "empty pool", "clamped grid", "unclamped grid", "refill of a running wave"]


def test_the_launches_reach_every_branch():
    log = set()
    per_run = {}
    for run in qc.runs():
        mine = set()
        walk(run, log=mine)
        per_run[run.name] = mine
        log |= mine
    missing = [b for b in REACH if b not in log]
    assert not missing, missing
    for b in REACH:
        print("%-36s %s" % (b, [n for n, m in per_run.items() if b in m][:4]))
    # 200 rays under one unit of 256 threads: four waves, several rounds each, pools of 50
    r = [x for x in qc.runs() if x.layout == "even" and x.grid_closest == 1 and x.grid_shadow == 1][0]
    assert r.n == 200 and max(1, BLOCK // TBLOCK) == 4 and (r.n + 3) // 4 == 50 and r.n > 4 * TQUADS


MUTANTS = ["<= for < in the fast path", "p5..p8 not collapsed", "first_cap dropped", "next + 16 for next + n_idle", "pool partition unclamped",
           "counter word off by one"]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_a_mutant_puts_a_ray_elsewhere(mutant):
    """Each mutant of the walk changes the place map of at least one launch: the GPU test's comparison of places, cells and
    counts would see the same mutant of the kernel."""
    changed = [run.name for run in qc.runs() if walk(run, mutant) != walk(run)]
    print(mutant, len(changed), changed[:6])
    assert changed, mutant


def test_the_first_clamp_alone_guards_nothing():
    """`min(n_sh, wave * per)` without the clamp: the pool's end is still clamped, a pool that begins behind it is empty, and no
    place changes -- the clamp that matters is the one of `first + per`, which the mutant above drops with it."""
    for run in qc.runs():
        assert walk(run, "wave * per unclamped, alone") == walk(run), run.name
