"""Seed -> the script of one animated application (tests/test_app_fuzz_gpu.py runs it through tests/app_model.py).  Pure numpy,
no GPU: tests/test_app_fuzz_cpu.py runs this generator alone and checks that the default seeds reach every operation and every
situation listed there, so that an edit here cannot quietly drop one.

A script is a dict: the scene, the frame size, the render config, the skins and morph targets registered before the first
operation, and `ops`, a list of OPS operations with all their arguments.  The first five operations of every script are a
frame whose post chain takes a temporal step with motion, three updates of one mesh by three different kinds (TRIPLES: over the
eight residues of the seed every ordered pair of kinds) and a second such frame, so the three updates share one temporal
interval; for seeds from 8 on the three kinds are drawn.  The other five operations are units (an operation, or a few that only mean
something side by side) drawn from the seed and put in a drawn order, under two caps: at most two refused calls, at least
three frame groups with a post chain.  The eight default seeds each carry some forced units (FORCED), so that together they
hold everything the CPU test lists whatever else they draw; their order is drawn too.

script(seed, late=True) is a second family over the seeds LATE_SEEDS (FOVPT_FUZZLATE_FROM / FOVPT_FUZZLATE_TO widen it), for what
the library has learnt since: the same scene, config, skins and morphs as the old script of that seed, a rig over them (make_rig),
and ten operations out of the old units and the new ones at the end of this file -- updates of kind "animated", "async" rebuilds
on all five kinds and with no entries, rebuild_state with its four flag values, set_rig, focus_reset, four more refused calls, and
a chain post -> focus -> expose -> packet (raw or coded) -> warp | warp_motion | lens.  script(seed) itself returns what it
always returned: tests/test_app_fuzz_cpu.py pins a digest of the scripts of seeds 0 .. 31.

script(seed, hdr=True) is a third family over HDR_SEEDS (FOVPT_FUZZHDR_FROM / FOVPT_FUZZHDR_TO widen it): the late script's scene,
size, config, skins, morphs and rig of that seed, and ten operations that put fovpt_variance, fovpt_variance_filter, fovpt_bloom and
fovpt_quality into the chain (see the section at the end of this file).  The late scripts and the hdr ones are pinned by digests too."""
import os

import numpy as np

import morph_ref as mr
import post_ref as po
import skin_ref as sk
import transform_ref as tf
from fovpathtracing_optixcodelatest_amd import abi, scenes

DEFAULT_SEEDS = range(0, 8)
SEEDS = range(int(os.environ.get("FOVPT_FUZZAPP_FROM", DEFAULT_SEEDS.start)), int(os.environ.get("FOVPT_FUZZAPP_TO", DEFAULT_SEEDS.stop)))  # widen for a sweep
OPS = 10
GATHER_BATCH = 32                                        # FOVPT_GATHER_BATCH
KINDS = ("vertices", "transforms", "skinned", "morphed")
# three kinds in turn on one mesh give the ordered pairs (a, b), (b, c), (a, c): the first six rows cover all twelve
TRIPLES = [(0, 1, 2), (2, 1, 0), (0, 3, 2), (2, 3, 0), (1, 3, 2), (2, 3, 1), (3, 0, 1), (1, 0, 3)]
# frame sizes, the families of postprocess_fuzz.EDGE_SHAPES within 130 x 90: one short of and one over a multiple of the 64-pixel
# tile with heights that are no multiple of 4, a frame narrower than one 4 x 4 block, and two ordinary ones
SIZES = [(63, 37), (65, 30), (127, 41), (129, 23), (3, 50), (96, 64), (64, 45)]
BIG = (192, 128)                                         # chains_per_frame = 2 needs 16384 sample slots
E_INVALID, E_NO_FRAME = -1, -5
F = np.float32

# The tail, operations 5 .. 9, is a shuffled list of UNITS: an operation, or a few that only mean something side by side.
# u: an update (kind, form, rebuild, "many": more meshes than one batch, "all": every mesh the kind can move); f: a frame group
# (frames, what runs between them, an update before the chain, the chain: None = drawn); x: a refused call; resize "same": to
# the size the frame has (the history and the frame as rendered go all the same), "other": to another size that has a packet.
U_SKINS = (("u", "skinned", "host", False), ("set_skins",), ("u", "skinned", "host", False, "all"))       # a pose, a new layout, every skin posed
U_MORPHS = (("u", "morphed", "host", False), ("set_morphs",))
U_RESIZE_SAME = (("resize", "same"), ("f", 1, (), False, "step"))
U_RESIZE_OTHER = (("resize", "other"), ("x", "no_frame"), ("u", "morphed+", "host", False), ("f", 1, (), False, "step+packet"))
U_RESIZE_FRAME = (("resize", "other"), ("f", 1, (), False, "step+packet"))
U_SCENE = (("set_scene",), ("x", "no_skin"), ("set_skins",))
U_RESET_FRAME = (("temporal_reset",), ("f", 1, (), True, None))
U_EXPOSE_RESET_FRAME = (("expose_reset",), ("f", 1, (), False, "expose"))
# the default seeds' units (the rest of their five operations is drawn like everybody's): together they hold every operation
# and situation tests/test_app_fuzz_cpu.py lists.  Seeds from 8 on draw all of theirs.
FORCED = [
    [U_SKINS, U_RESIZE_SAME],
    [(("f", 3, ("u", "x:overflow"), False, None),), (("expose_reset",),), U_RESET_FRAME, (("u", "morphed+", "host", True),)],
    [(("u", "vertices", "host", False, "many"),), U_MORPHS, (("f", 2, (None,), False, None),), (("u", "vertices", "device", True),)],
    [(("f", 2, ("x:mesh_range",), False, None),), U_SCENE],
    [(("f", 1, (), True, "step"),), U_RESIZE_OTHER],
    [(("u", "transforms", "host", True, "many"),), (("f", 2, ("u",), False, None),), (("x", "overflow"),), (("u", "morphed", "device", False),)],
    [(("u", "skinned", "device", True),), (("f", 1, (), False, "packet"),), U_EXPOSE_RESET_FRAME, (("u", "morphed+", "device", False),)],
    [(("u", "empty", "host", False),), (("set_morphs",),), (("u", "transforms", "host", True),), (("x", "overflow"),), (("f", 3, (None, "u"), True, None),)],
]
TAIL_OPS = 5
MAX_REFUSED = 2


def scene_of(s):
    """(model, camera) of a script."""
    if s["scene"][0] == "cornell":
        return scenes.cornell_box(), scenes.CORNELL_CAMERA
    return scenes.atrium(s["scene"][1]), scenes.ATRIUM_CAMERA


class _Draw:
    """The generator's state: what is registered, so that every pose drawn as valid fits the layout it will meet."""

    def __init__(self, seed):
        self.seed, self.m = seed, seed % 8
        self.rng = np.random.default_rng(52000 + seed)
        rng = self.rng
        atrium = self.m in (2, 5)
        self.s = dict(seed=seed, scene=("atrium", int(rng.integers(500, 2001))) if atrium else ("cornell",))
        self.model, self.cam = scene_of(self.s)
        self.nmesh = len(self.model.meshes)
        self.nv = [m.vertex.shape[0] for m in self.model.meshes]
        chains = self.m % 4 == 3
        self.s["size"] = self.size = BIG if chains else SIZES[int(rng.integers(0, len(SIZES)))]
        uniform = int(rng.random() < 0.25)
        ri = int(rng.integers(0, 30))
        cfg = dict(uniform=uniform, r_inner=ri, r_outer=ri + int(rng.integers(1, 50)), spp=tuple(int(x) for x in rng.integers(1, 5, 4)),
                   max_depth=int(rng.integers(1, 4)), frames_in_flight=2 if self.m % 4 == 1 else 0, chains_per_frame=2 if chains else 0)
        if chains:                                      # a fovea of 4 samples over more than 4096 pixels: >= 16384 sample slots
            cfg.update(uniform=0, r_inner=40, r_outer=40 + int(rng.integers(1, 40)), spp=(int(rng.integers(1, 5)), int(rng.integers(1, 5)), 4, 4))
        self.s["config"] = cfg
        t = dict(zip(("history_fovea", "history_middle", "history_periphery", "history_uniform"), (int(x) for x in rng.choice([2, 3, 8, abi.TEMPORAL_MAX_HISTORY], 4))))
        self.s["post"] = dict(denoise=dict(iterations_fovea=int(rng.integers(0, 2)), iterations_middle=int(rng.integers(0, 3)),
                                           iterations_periphery=int(rng.integers(0, 3)), iterations_uniform=int(rng.integers(0, 3))),
                              reconstruct=dict(levels=int(rng.integers(0, 3))), temporal=t)
        # the meshes that pose: on the Cornell box the two blocks (3, 4), the floor and a wall; in the atrium the first 48
        self.posable = [4, 3, 0, 5] if not atrium else list(range(48))
        self.x = self.posable[0] if not atrium else int(rng.integers(0, 40))       # the mesh of the interval's three updates
        self.skins = {k: self.skin(k) for k in self.posable}
        self.morphs = {k: self.targets(k) for k in self.posable[:-1]}          # (one left for a set_morphs to add)
        self.s["skins"], self.s["morphs"] = dict(self.skins), dict(self.morphs)
        self.frames = 0

    # ---- what gets registered
    def skin(self, k):
        return sk.random_skin(self.rng, self.nv[k], int(self.rng.integers(1, 6)))

    def targets(self, k):
        nt = int(self.rng.integers(1, 5))
        t = mr.random_targets(self.rng, self.nv[k], nt, dense=int(self.rng.integers(0, 2)), fraction=0.5, scale=12.0)
        if all(mr.split(x, self.nv[k])[1].size == 0 or not np.abs(mr.split(x, self.nv[k])[1]).max() >= 1 for x in t):
            t[0] = np.full((self.nv[k], 3), 2.0, F)     # (some delta of at least 1: a weight of 3e38 then overflows)
        return t

    # ---- poses
    def centre(self, k):
        return self.model.meshes[k].vertex.astype(np.float64).mean(axis=0)

    def pose(self, kind, k):
        rng, v = self.rng, self.model.meshes[k].vertex
        if kind == "vertices":
            return (v + rng.uniform(-6.0, 6.0, v.shape).astype(F)).astype(F)
        if kind == "transforms":
            return tf.rotation_translation(rng.uniform(-25, 25), self.centre(k), rng.uniform(-12, 12, 3))
        if kind == "skinned":
            return sk.random_pose(rng, v, self.skins[k][2])
        w = mr.random_weights(rng, len(self.morphs[k]), active=0.7)
        return (w, sk.random_pose(rng, v, self.skins[k][2])) if kind == "morphed+" else w

    def meshes_for(self, kind, many=False):
        """The meshes one call moves: a random subset of those the kind can move, more than GATHER_BATCH with many."""
        rng = self.rng
        if kind in ("vertices", "transforms"):
            pool = list(range(self.nmesh))
        elif kind == "skinned":
            pool = sorted(self.skins)
        elif kind == "morphed":
            pool = sorted(self.morphs)
        else:
            pool = sorted(set(self.skins) & set(self.morphs))
        if many == "all":
            return pool
        if many and len(pool) > GATHER_BATCH:
            n = int(rng.integers(GATHER_BATCH + 1, min(len(pool), 2 * GATHER_BATCH + 8) + 1))
        else:
            n = int(rng.integers(1, min(len(pool), 5) + 1)) if pool else 0
        return sorted(int(k) for k in rng.choice(pool, n, replace=False)) if n else []

    def update(self, kind, form="host", rebuild=False, many=False, meshes=None):
        if kind == "empty":
            kind, meshes = KINDS[int(self.rng.integers(0, 4))], []
        meshes = self.meshes_for(kind, many) if meshes is None else meshes
        base = "morphed" if kind == "morphed+" else kind
        return dict(op="update", kind=base, poses={k: self.pose(kind, k) for k in meshes}, rebuild=bool(rebuild),
                    device=form == "device" and base != "transforms")

    def refused(self, which):
        rng = self.rng
        if which == "overflow":
            kinds = [k for k in KINDS[1:] if k == "transforms" or (self.skins if k == "skinned" else self.morphs)]
            kind = kinds[int(rng.integers(0, len(kinds)))]
            k = self.meshes_for(kind)[0]
            p = self.pose(kind, k)
            if kind == "morphed":
                p = p.copy()
                t = int(np.argmax(mr.target_max(self.morphs[k], self.nv[k])))
                p[t] = F(3e38)
            else:
                p = np.array(p, F)
                p[..., int(rng.integers(0, 3)), 3] = F(-3e38)
            good = self.meshes_for(kind)
            poses = {g: self.pose(kind, g) for g in good if g != k}             # good poses beside the bad one: all or nothing
            poses[k] = p
            return dict(op="refused", which=which, kind=kind, poses=poses, bad=k, code=E_INVALID)
        if which == "mesh_range":
            kinds = [k for k in KINDS if k in ("vertices", "transforms") or (self.skins if k == "skinned" else self.morphs)]
            kind = kinds[int(rng.integers(0, len(kinds)))]
            k = self.meshes_for(kind)[0]
            bad = self.nmesh if rng.random() < 0.5 else -1
            return dict(op="refused", which=which, kind=kind, poses={bad: self.pose(kind, k)}, bad=bad, code=E_INVALID)
        if which == "no_skin":
            bare = [k for k in range(self.nmesh) if k not in self.skins]
            k = int(rng.choice(bare))
            return dict(op="refused", which=which, kind="skinned", poses={k: np.stack([tf.IDENTITY] * 2)}, bad=k, code=E_INVALID)
        assert which == "no_frame"
        return dict(op="refused", which=which, calls=("post", "expose", "packet"), code=E_NO_FRAME)      # each of the three

    # ---- registration
    def set_skins(self):
        """One call that replaces, removes and adds: the lowest skinned mesh gets a skin of more joints (every later mesh's place
        in the palette buffer moves up), the highest but one another joint count, the highest goes (three or more skinned), and
        one mesh without a skin gets one."""
        rng, new = self.rng, {}
        have = sorted(self.skins)
        bare = [k for k in self.posable if k not in self.skins]
        if len(have) >= 3 and have[-1] != self.x:
            new[have.pop()] = None
        if have:
            k = have[0]
            new[k] = sk.random_skin(rng, self.nv[k], self.skins[k][2] + int(rng.integers(1, 3)))
        if len(have) >= 2:
            k = have[-1]
            new[k] = self.skin(k)
            while new[k][2] == self.skins[k][2]:
                new[k] = self.skin(k)
        if bare:
            k = bare[int(rng.integers(0, len(bare)))]
            new[k] = self.skin(k)
        for k, v in new.items():
            if v is None:
                self.skins.pop(k, None)
            else:
                self.skins[k] = v
        return dict(op="set_skins", skins=new)

    def set_morphs(self):
        rng, new = self.rng, {}
        have = sorted(self.morphs)
        bare = [k for k in self.posable if k not in self.morphs]
        if have:
            new[have[int(rng.integers(0, len(have)))]] = "replace"
        rest = [k for k in have if k not in new and k != self.x]
        if rest:
            new[rest[int(rng.integers(0, len(rest)))]] = None
        if bare:
            new[bare[int(rng.integers(0, len(bare)))]] = "add"
        for k, v in list(new.items()):
            if v is not None:
                old = self.morphs.get(k)
                new[k] = self.targets(k)
                while old is not None and len(new[k]) == len(old):
                    new[k] = self.targets(k)
        for k, v in new.items():
            if v is None:
                self.morphs.pop(k, None)
            else:
                self.morphs[k] = v
        return dict(op="set_morphs", morphs=new)

    # ---- frames
    def expose_config(self):
        rng = self.rng
        lo = int(rng.integers(0, 1000))
        ev = np.sort(rng.uniform(-16, 16, 2)).astype(F)
        d = dict(mode=int(rng.random() < 0.85), metering=int(rng.integers(0, 2)), tone=int(rng.integers(0, 2)),
                 low_permille=lo, high_permille=int(rng.integers(lo + 1, 1001)), ev_min=float(ev[0]), ev_max=float(ev[1]),
                 key=float(F(np.exp2(rng.uniform(-8, 8)))), exposure=float(F(np.exp2(rng.uniform(-8, 8)))), white=float(F(np.exp2(rng.uniform(-4, 19)))),
                 adapt_brighter=float(F(rng.uniform(0.01, 1.0))), adapt_darker=float(F(rng.uniform(0.01, 1.0))))
        for k in ("weight_fovea", "weight_middle", "weight_periphery", "weight_uniform"):
            d[k] = int(rng.choice([0, 1, 255, int(rng.integers(0, 256))]))
        return d

    def chain(self, want=None):
        """dict(post=stage mask or None, expose=config or None, packet=bool): want "step" forces a temporal step with motion,
        "packet" / "expose" that stage alone; otherwise each stage is there or not, at least one."""
        rng = self.rng
        if want == "packet":
            return dict(post=None, expose=None, packet=True)
        if want == "expose":
            return dict(post=None, expose=self.expose_config(), packet=False)
        step = want in ("step", "step+packet")
        masks = [s for s in po.VALID_STAGES if not step or (s & po.TEMPORAL and s & po.MOTION)]
        c = dict(post=masks[int(rng.integers(0, len(masks)))] if step or rng.random() < 0.8 else None,
                 expose=self.expose_config() if rng.random() < 0.6 else None, packet=bool(want == "step+packet" or rng.random() < 0.6))
        if c["post"] is None and c["expose"] is None and not c["packet"]:
            c["post"] = masks[int(rng.integers(0, len(masks)))]
        return c

    def frame(self, n=1, between=(), pre_chain=False, want=None):
        rng = self.rng
        w, h = self.size
        views = [dict(gaze=(int(rng.integers(-10, w + 11)), int(rng.integers(-10, h + 11))), subframe_index=int(rng.integers(0, 4)),
                      eye=tuple(float(x) for x in rng.uniform(-0.02, 0.02, 3))) for _ in range(n)]
        mid = []
        for b in between:
            if b is None:
                mid.append(None)
            elif b == "u":
                kind = ("vertices", "transforms", "skinned", "morphed", "morphed+")[int(rng.integers(0, 5))]
                mid.append(self.update(kind, "device" if rng.random() < 0.4 else "host"))
            else:
                mid.append(self.refused(b[2:]))
        pre = self.update(KINDS[int(rng.integers(0, 4))], "host") if pre_chain else None
        self.frames += 1
        # the caller's next gaze and subframe index, written into the launch parameters between the render and its chain
        moved_on = dict(gaze=(int(rng.integers(-10, w + 11)), int(rng.integers(-10, h + 11))), subframe_index=int(rng.integers(4, 9))) \
            if pre_chain or rng.random() < 0.5 else None
        return dict(op="frame", views=views, between=mid, pre_chain=pre, chain=self.chain(want), moved_on=moved_on,
                    sync=bool(n == 1 and (self.seed + self.frames) % 2 == 0))

    def resize(self, how=None):
        rng = self.rng
        if how is None:
            how = "same" if rng.random() < 0.25 else "any"
        pool = [x for x in SIZES if (x == self.size) == (how == "same") and (how != "other" or x[0] >= 4)] or [self.size]
        self.size = pool[int(rng.integers(0, len(pool)))]
        return dict(op="resize", size=self.size)

    def set_scene(self):
        self.skins, self.morphs = {}, {}
        return dict(op="set_scene")

    def expose_reset(self):
        return dict(op="expose_reset")

    def temporal_reset(self):
        return dict(op="temporal_reset")

    def draw_unit(self, room):
        """One unit of at most `room` operations, drawn."""
        rng = self.rng
        while True:
            u = rng.random()
            if u < 0.30:
                kind = ("vertices", "transforms", "skinned", "morphed", "morphed+", "empty")[int(rng.integers(0, 6))]
                unit = (("u", kind, "device" if rng.random() < 0.4 else "host", bool(rng.random() < 0.3)) + (("many",) if rng.random() < 0.2 else ()),)
            elif u < 0.55:
                n = int(rng.integers(1, 4))
                between = tuple((None, "u", "u", "x:overflow", "x:mesh_range")[int(rng.integers(0, 5))] for _ in range(n - 1))
                unit = (("f", n, between, bool(rng.random() < 0.4), None),)
            elif u < 0.70:
                unit = (U_SKINS, U_MORPHS, (("set_skins",),), (("set_morphs",),))[int(rng.integers(0, 4))]
            elif u < 0.85:
                unit = (U_RESIZE_SAME, U_RESIZE_OTHER, U_RESIZE_FRAME, U_RESIZE_FRAME, (("resize",),))[int(rng.integers(0, 5))]
            elif u < 0.90:
                unit = U_SCENE if rng.random() < 0.5 else (("set_scene",),)
            elif u < 0.95:
                unit = ((("x", "overflow"),), (("x", "mesh_range"),), (("x", "no_skin"),))[int(rng.integers(0, 3))]
            else:
                unit = (U_RESET_FRAME, U_EXPOSE_RESET_FRAME, (("temporal_reset",),), (("expose_reset",),))[int(rng.integers(0, 4))]
            if len(unit) <= room:
                return unit

    def realize(self, t):
        """One operation of a unit, with its arguments drawn against the state the operations before it leave."""
        if t[0] == "x" or (t[0] == "f" and any(b and b.startswith("x:") for b in t[2])):
            if t[0] == "x":
                if self.refusals >= MAX_REFUSED or (t[1] == "no_frame" and not self.resized):
                    return self.temporal_reset()                 # (the cap is reached: something harmless in its place)
                self.refusals += 1
                return self.refused(t[1])
            between = []
            for b in t[2]:
                if b and b.startswith("x:") and self.refusals >= MAX_REFUSED:
                    b = None
                self.refusals += bool(b and b.startswith("x:"))
                between.append(b)
            t = t[:2] + (tuple(between),) + t[3:]
        self.resized = t[0] == "resize"
        if t[0] == "u":
            return self.update(t[1], t[2], t[3], many=t[4] if len(t) > 4 else False)
        if t[0] == "f":
            return self.frame(t[1], t[2], t[3], t[4])
        return getattr(self, t[0])(*t[1:])

    def script(self):
        rng = self.rng
        default = self.seed in DEFAULT_SEEDS
        a, b, c = (KINDS[k] for k in (TRIPLES[self.seed] if default else rng.permutation(4)[:3]))

        def burst(kind, last):
            form = "device" if kind != "transforms" and rng.random() < 0.4 else "host"
            k = "morphed+" if kind == "morphed" and rng.random() < 0.5 else kind
            others = [g for g in self.meshes_for(k) if g != self.x][:2]
            return self.update(k, form, rebuild=last and (self.m % 2 == 0 if default else rng.random() < 0.5), meshes=sorted([self.x] + others))
        self.refusals, self.resized = 0, False
        ops = [self.frame(want="step"), burst(a, False), burst(b, False), burst(c, True), self.frame(want="step")]
        # the tail: the forced units of a default seed, drawn ones up to five operations, a frame group among them, in drawn order
        units = list(FORCED[self.seed]) if default else []
        room = TAIL_OPS - sum(len(u) for u in units)
        if not any(t[0] == "f" for u in units for t in u):
            n = int(rng.integers(1, 4))
            units.append((("f", n, (None,) * (n - 1), bool(rng.random() < 0.4), None),))
            room -= 1
        while room > 0:
            units.append(self.draw_unit(room))
            room -= len(units[-1])
        for k in rng.permutation(len(units)):
            ops += [self.realize(t) for t in units[k]]
        assert len(ops) == OPS
        self.s["ops"] = ops
        return self.s


# ---- the late family: rigs, background rebuilds, focus, warp, warp_motion, lens, coded packets -------------------------------
# A late script has the shape of an old one and one entry more, the rig registered after the skins and morphs.  Its operations
# are the old ones and: update of kind "animated" (poses = dict(clip, time)); rebuild "async" beside False and True on any update;
# rebuild_state(wait, adopt); set_rig; focus_reset; the refusals no_rig, clip_range, async_with_rebuild, warp_motion_stale; and a
# chain post -> focus -> expose -> packet (raw or coded, of the unwarped frame) -> warp | warp_motion | lens.
LATE_DEFAULT_SEEDS = range(0, 8)
LATE_SEEDS = range(int(os.environ.get("FOVPT_FUZZLATE_FROM", LATE_DEFAULT_SEEDS.start)), int(os.environ.get("FOVPT_FUZZLATE_TO", LATE_DEFAULT_SEEDS.stop)))
LATE_KINDS = KINDS + ("animated",)
# the three kinds of the head's interval: the first four rows hold the eight ordered pairs of "animated" (4) with another kind
LATE_TRIPLES = [(0, 4, 1), (2, 4, 3), (1, 4, 0), (3, 4, 2), (4, 2, 1), (3, 1, 4), (0, 4, 3), (1, 2, 4)]
# the flags of the head's three updates: background builds left in flight, and (4) one ended by FOVPT_UPDATE_REBUILD
LATE_HEAD_FLAG = [(False, False, "async"), (False, False, "async"), (False, False, "async"), (False, False, "async"),
                  (False, "async", True), (False, False, "async"), (False, False, False), (False, False, True)]
ADVANCES = (0.0, 0.5, 1.0, 2.0)
# clip times against the keys 0, 0.5, 1, 2: before the first, between (the lerp, the flipped slerp and the slerp segment of a
# rotation channel), exactly a key, behind the last
CLIP_TIMES = (-0.5, 0.25, 0.5, 0.75, 1.5, 3.0)
ROT_KEYS = (0.0, 0.5, 1.0, 2.0)
RAW, BC1, BY_FILL = 0, 1, 0xffffffff
FIXED, AUTO = 0, 1
T_, M_ = po.TEMPORAL, po.MOTION

L_NO_RIG = lambda drop: ((drop,), ("x", "no_rig"), ("set_rig",), ("u", "animated", "host", False))
# the late default seeds' units; a chain given as a dict is forced stage by stage (late_chain)
LATE_FORCED = [
    # 0: adoption by a later update after WAIT, inside a tracked interval; focus AUTO across a resize
    [(("u", "empty", "host", "async"), ("rebuild_state", True, False), ("u", "vertices", "host", False)),
     (("resize", "other"), ("f", 1, (), False, dict(step=True, focus=(AUTO, "temporal"), last=("warp_motion", "temporal", 2.0), codec=(BC1, RAW, BY_FILL))))],
    # 1: set_skins drops the rig; a stale snapshot adopted by rebuild_state (the script widens the BUILDING window)
    [L_NO_RIG("set_skins"),
     (("f", 3, ("u:async", "u"), False, dict(step=True, adopt_first=True, focus=(FIXED, "own"), last=("lens", 0, True))),)],
    # 2: a request while a build is in flight; an adopting update between two frames in flight
    [(("u", "skinned", "host", "async"), ("u", "empty", "host", "async"), ("rebuild_state", True, False), ("f", 2, ("u",), False, dict(step=True, last=("lens", 1, False)))),],
    # 3: set_morphs drops the rig
    [L_NO_RIG("set_morphs"), (("f", 1, (), False, dict(step=True, focus=(AUTO, "own"), last=("warp",), codec=(BY_FILL, BY_FILL, BY_FILL))),)],
    # 4: set_scene drops the rig and ends a build; the step after it did not know the motion
    [(("u", "vertices", "host", "async"),) + L_NO_RIG("set_scene")[:3] + (("f", 1, (), "animated", dict(step=True, last=("warp_motion", "own", 1.0), codec=(BC1, BC1, BC1))),)],
    # 5: warp_motion refused after an update; rebuild_state polled and with ADOPT alone
    [(("f", 1, (), False, dict(step=True, last=("warp_motion", "own", 0.0))), ("u", "transforms", "host", False), ("x", "warp_motion_stale")),
     (("rebuild_state", False, False),), (("rebuild_state", False, True),)],
    # 6: both rebuild flags; a clip out of range; focus_reset
    [(("x", "async_with_rebuild"),), (("focus_reset",), ("f", 1, (), False, dict(focus=(AUTO, "own"), last=("lens", 2, True)))),
     (("x", "clip_range"),), (("f", 1, (), False, dict(last=("lens", 0, False), codec=(RAW, BC1, RAW))),)],
    # 7: rebuild_state(WAIT | ADOPT) as an operation of its own
    [(("u", "animated", "host", "async"), ("rebuild_state", True, True)), (("f", 1, (), False, dict(last=("lens", 1, True))),)],
]
# the chain of the head's second frame: the stale G-buffer (seeds whose head leaves a build in flight), every advance
LATE_HEAD_CHAIN = [
    dict(step=True, focus=(AUTO, "temporal"), last=("warp_motion", "temporal", 1.0, "adopt"), codec=(BY_FILL, BC1, RAW)),
    dict(step=True, last=("warp_motion", "own", 0.5)),
    dict(step=True, focus=(AUTO, "temporal"), last=("warp_motion", "temporal", 2.0)),
    dict(step=True, focus=(FIXED, "temporal"), last=("warp_motion", "temporal", 1.0, "adopt"), codec=(BC1, BC1, RAW)),
    dict(step=True, last=("warp_motion", "own", 2.0)),
    dict(step=True, last=("lens", 2, False)),
    dict(step=True, last=("warp_motion", "own", 0.0)),
    dict(step=True, focus=(AUTO, "own"), last=("warp_motion", "temporal", 1.0)),
]
LATE_DELAY_MS = {1: 150}                                  # FOVPT_ASYNC_BUILD_DELAY_MS of a script: widens a window, decides nothing


class _LateDraw(_Draw):
    def __init__(self, seed):
        super().__init__(seed)
        self.rng = np.random.default_rng(53000 + seed)   # (the scene, config, skins and morphs are the old family's of this seed)
        if seed in LATE_DEFAULT_SEEDS and self.s["config"]["chains_per_frame"] == 0:
            self.s["size"] = self.size = SIZES[seed % len(SIZES)]     # every size of the pool, (3, 50) among them
        self.s["late"] = True
        self.s["delay_ms"] = LATE_DELAY_MS.get(seed, 0) if seed in LATE_DEFAULT_SEEDS else 0
        self.rig = self.make_rig()
        self.s["rig"] = self.rig
        self.stepped = False                              # a temporal step at this size, on this scene, since the last reset
        self.posed = 0                                    # animated updates so far

    # ---- the rig
    def make_rig(self):
        """A rig over the registered skins and morphs: the mesh of the interval's updates morphed and skinned, one mesh by morph
        weights alone, one skinned, one or two rigid; a root, a pivot per mesh at its centre and chains of joints below the pivots
        (four levels and more); clip 0 with STEP and LINEAR channels of all four paths, rotation keys 2 degrees apart (the lerp),
        on opposite hemispheres (the flip) and 20 degrees apart (the slerp); clip 1 carries the root alone."""
        import rig_ref as rg
        rng = self.rng
        both = [k for k in sorted(self.skins) if k in self.morphs]
        bind = [(self.x, "morph+skin")] if self.x in both else []
        rest = [k for k in both if k != self.x]
        bind += [(k, "morph") for k in rest[:1]] + [(k, "morph+skin") for k in rest[1:2]]
        bind += [(k, "skin") for k in [k for k in sorted(self.skins) if k not in self.morphs][:1]]
        bind += [(k, "morph") for k in [k for k in sorted(self.morphs) if k not in self.skins][:1]]
        taken = {k for k, _ in bind}
        bare = [k for k in range(self.nmesh) if k not in taken and k not in self.morphs and k not in self.skins]
        bind += [(k, "rigid") for k in ([self.x] if self.x not in taken and self.x not in self.morphs else []) + bare[:1 if taken else 2]]
        parent, trans = [-1], [np.zeros(3)]
        bindings, clip, count = [], [], [0, 0, 0, 0]

        def node(p, t):
            parent.append(p)
            trans.append(np.asarray(t, np.float64))
            return len(parent) - 1

        def chan(target, path, times, values):
            count[path] += 1
            clip.append(rg.channel(target, path, times, values, rg.STEP if count[path] % 3 == 2 else rg.LINEAR))

        def turns(target):
            axis, axis2 = rng.standard_normal(3), rng.standard_normal(3)
            a = rng.uniform(-5, 5)
            q = [rg.quat(axis, a), rg.quat(axis, a + 2.0), -rg.quat(axis2, a + 20.0), -rg.quat(axis2, a + 40.0)]
            chan(target, rg.ROTATION, ROT_KEYS, q)

        joints = {}
        for k, how in bind:
            c = self.centre(k)
            p = node(0, c)
            chan(p, rg.TRANSLATION, [0.0, 1.0, 2.0], c[None, :] + rng.uniform(-8, 8, (3, 3)))
            if how == "rigid":
                n = node(p, -c)
                turns(p)
                chan(n, rg.SCALE, [0.5, 1.5], rng.uniform(0.9, 1.1, (2, 3)))
                bindings.append(dict(mesh=k, node=n))
            elif how == "morph":
                bindings.append(dict(mesh=k))
            else:
                js = []
                for j in range(self.skins[k][2]):
                    js.append(node(js[-1] if j % 3 else p, rng.uniform(-4, 4, 3)))
                    if j < 3:
                        turns(js[-1])
                chan(js[0], rg.SCALE, [0.5, 1.5], rng.uniform(0.9, 1.1, (2, 3)))
                joints[k] = js
                bindings.append(dict(mesh=k, joint_nodes=np.array(js, np.uint16)))
            if k in self.morphs:
                chan(k, rg.WEIGHTS, ROT_KEYS, rng.uniform(-0.5, 1.0, (4, len(self.morphs[k]))))
        rig = rg.empty_rig(len(parent))
        rig["parent"] = np.array(parent, np.int32)
        rig["translation"] = np.array(trans).astype(F)
        for b in bindings:
            if "joint_nodes" in b:
                b["inverse_bind"] = rg.inverse_bind_of(rig, b["joint_nodes"])
        rig["bindings"] = bindings
        rig["clips"] = [clip, [rg.channel(0, rg.TRANSLATION, [0.0, 1.0], [[0, 0, 0], rng.uniform(-6, 6, 3)])]]
        return rig

    def set_rig(self):
        self.rig = self.make_rig()
        return dict(op="set_rig", rig=self.rig)

    def set_skins(self):
        self.rig = None
        return super().set_skins()

    def set_morphs(self):
        self.rig = None
        return super().set_morphs()

    def set_scene(self):
        self.rig, self.stepped = None, False
        return super().set_scene()

    def resize(self, how=None):
        self.stepped = False
        return super().resize(how)

    def temporal_reset(self):
        self.stepped = False
        return super().temporal_reset()

    def focus_reset(self):
        return dict(op="focus_reset")

    def rebuild_state(self, wait, adopt):
        return dict(op="rebuild_state", wait=bool(wait), adopt=bool(adopt))

    # ---- updates
    def update(self, kind, form="host", rebuild=False, many=False, meshes=None):
        rng = self.rng
        flag = rebuild if rebuild == "async" else bool(rebuild)
        if kind == "animated" and self.rig is None:
            kind = "vertices"                             # (the rig went: something that still moves)
        if kind == "animated":
            clip = int(rng.random() < 0.2)
            t = int(rng.integers(0, len(CLIP_TIMES)))
            if self.seed in LATE_DEFAULT_SEEDS:           # the default seeds take the times in turn: every case of the sample rule
                t, self.posed = (self.seed + self.posed) % len(CLIP_TIMES), self.posed + 1
                clip = clip if self.posed > 1 else 0
            return dict(op="update", kind="animated", poses=dict(clip=clip, time=float(CLIP_TIMES[t])),
                        rebuild=flag, device=False)
        u = super().update(kind, form, False, many, meshes)
        u["rebuild"] = flag
        return u

    def refused(self, which):
        rng = self.rng
        T = float(rng.uniform(0.0, 2.0))
        if which == "no_rig":
            assert self.rig is None
            return dict(op="refused", which=which, clip=0, time=T, code=E_INVALID)
        if which == "clip_range":
            return dict(op="refused", which=which, clip=len(self.rig["clips"]) if rng.random() < 0.5 else -1, time=T, code=E_INVALID)
        if which == "async_with_rebuild":
            return dict(op="refused", which=which, kind="animated" if self.rig is not None and rng.random() < 0.5 else "vertices", clip=0, time=T, code=E_INVALID)
        if which == "warp_motion_stale":
            return dict(op="refused", which=which, to=self.newer_camera(), code=E_NO_FRAME)
        return super().refused(which)

    # ---- the chain
    def newer_camera(self):
        """(how, eye, lookat) of a camera a little later: a slide, a turn or a dolly of the script's."""
        rng = self.rng
        eye, look = np.array(self.cam["eye"], np.float64), np.array(self.cam["lookat"], np.float64)
        d = np.linalg.norm(look - eye)
        how = ("slide", "turn", "dolly")[int(rng.integers(0, 3))]
        off = rng.uniform(-1, 1, 3) * 0.04 * d
        if how == "slide":
            eye, look = eye + off, look + off
        elif how == "turn":
            look = look + 3 * off
        else:
            eye = eye + (look - eye) * rng.uniform(-0.15, 0.15)
        return (how, tuple(float(x) for x in eye), tuple(float(x) for x in look))

    def focus_config(self, mode, gbuffer):
        rng = self.rng
        d = float(np.linalg.norm(np.array(self.cam["lookat"], np.float64) - np.array(self.cam["eye"], np.float64)))
        return dict(mode=int(mode), gbuffer=gbuffer, meter_radius=int(rng.integers(8, 41)), rank_permille=int(rng.integers(0, 1001)),
                    max_radius=int(rng.integers(1, 6)), strength=float(F(d * rng.uniform(4, 30))), focus_distance=float(F(d * rng.uniform(0.6, 1.4))),
                    focus_default=float(F(d)), adapt_nearer=float(F(rng.uniform(0.1, 1.0))), adapt_farther=float(F(rng.uniform(0.1, 1.0))))

    def late_chain(self, want):
        """dict(post, expose, packet, codec, focus, last) -- the stages in the order they run; want forces the entries it names:
        step (a temporal step with motion), focus (mode, gbuffer), last (stage, ...), codec (a triple; "raw"; None: no packet)."""
        rng = self.rng
        want = dict(want or {})
        draw_last = "last" not in want
        if draw_last:
            want["last"] = ((None,), ("warp",), ("warp_motion", "own" if rng.random() < 0.5 else "temporal", ADVANCES[int(rng.integers(0, 4))]),
                            ("lens", int(rng.integers(0, 3)), bool(rng.random() < 0.5)))[int(rng.integers(0, 4))]
        if "focus" not in want:
            want["focus"] = (int(rng.integers(0, 2)), "own" if rng.random() < 0.5 else "temporal") if rng.random() < 0.4 else None
        last, focus = want["last"], want["focus"]
        step = bool(want.get("step") or last[0] == "warp_motion" or (focus and focus[1] == "temporal"))
        masks = [s for s in po.VALID_STAGES if not step or (s & T_ and s & M_)]
        post = masks[int(rng.integers(0, len(masks)))] if step or rng.random() < 0.8 else None
        c = dict(post=post, expose=self.expose_config() if rng.random() < 0.5 else None, packet=False, codec=None, focus=None, last=None)
        if "codec" not in want:
            want["codec"] = (None, "raw", tuple(int(x) for x in rng.choice([RAW, BC1, BY_FILL], 3)))[int(rng.integers(0, 3))]
        if want["codec"] is not None:
            c["packet"] = True
            c["codec"] = None if want["codec"] == "raw" else tuple(int(k) for k in want["codec"])
        if focus:
            c["focus"] = self.focus_config(*focus)
        if last[0] in ("warp", "warp_motion"):
            c["last"] = dict(stage=last[0], to=self.newer_camera(), images=int(rng.integers(1, 4)), fill_radius=int(rng.integers(0, 4)))
            if last[0] == "warp_motion":
                c["last"].update(gbuffer=last[1], advance=float(last[2]), adopt=len(last) > 3)
        elif last[0] == "lens":
            c["last"] = dict(stage="lens", filter=int(last[1]), to=self.newer_camera() if last[2] else None,
                             chroma=tuple(float(F(x)) for x in (rng.uniform(0.95, 1.0), 1.0, rng.uniform(1.0, 1.05))))
        if post is not None and post & T_:
            self.stepped = True
        return c

    def frame(self, n=1, between=(), pre_chain=False, want=None):
        flags = [b[2:] if isinstance(b, str) and b.startswith("u:") else None for b in between]
        # (the old frame with the cheapest chain there is, "packet": its views, between and moved_on are kept, the chain it drew
        # is thrown away on purpose and late_chain() draws the one that runs)
        op = super().frame(n, tuple("u" if f else b for f, b in zip(flags, between)), False, "packet")
        for k, f in enumerate(flags):
            if f:
                op["between"][k]["rebuild"] = f
        if pre_chain:
            kind = pre_chain if isinstance(pre_chain, str) else LATE_KINDS[int(self.rng.integers(0, 5))]
            op["pre_chain"] = self.update(kind, "host")
            if op["moved_on"] is None:
                w, h = self.size
                op["moved_on"] = dict(gaze=(int(self.rng.integers(-10, w + 11)), int(self.rng.integers(-10, h + 11))), subframe_index=int(self.rng.integers(4, 9)))
        adopt_first = isinstance(want, dict) and want.pop("adopt_first", False)
        op["chain"] = self.late_chain(want if isinstance(want, dict) else dict(step=True) if want in ("step", "step+packet") else None)
        op["adopt_first"] = bool(adopt_first)             # rebuild_state(WAIT | ADOPT) between the frames and their chain
        return op

    def draw_unit(self, room):
        rng = self.rng
        while True:
            u = rng.random()
            if u < 0.45:
                unit = super().draw_unit(room)
            elif u < 0.65:
                flag = (False, True, "async", "async")[int(rng.integers(0, 4))]
                kind = ("animated", "animated", "vertices", "transforms", "skinned", "morphed", "empty")[int(rng.integers(0, 7))]
                unit = (("u", kind, "host", flag),)
            elif u < 0.80:
                unit = (("rebuild_state", bool(rng.random() < 0.5), bool(rng.random() < 0.5)),)
            elif u < 0.85:
                unit = (("u", "animated", "host", "async"), ("rebuild_state", True, False), ("u", "animated", "host", False))
            elif u < 0.90:
                unit = (("focus_reset",),)
            elif u < 0.95:
                unit = ((("x", "clip_range"),), (("x", "async_with_rebuild"),), L_NO_RIG("set_skins"), L_NO_RIG("set_morphs"))[int(rng.integers(0, 4))]
            else:
                unit = (("f", 1, (), False, dict(step=True)), ("u", "vertices", "host", False), ("x", "warp_motion_stale"))
            if len(unit) <= room:
                return unit

    def realize(self, t):
        if t[0] == "x" and t[1] in ("no_rig", "clip_range", "warp_motion_stale") and self.refusals < MAX_REFUSED:
            if (t[1] == "no_rig") != (self.rig is None) or (t[1] == "warp_motion_stale" and not self.stepped):
                return self.temporal_reset()                 # (nothing to refuse here: something harmless in its place)
        if t[0] == "set_rig" and self.rig is not None:
            return self.focus_reset()
        return super().realize(t)

    def tables(self):
        """(the default seeds, the flags of their heads' updates, their forced units): what a family built on this one replaces."""
        return LATE_DEFAULT_SEEDS, LATE_HEAD_FLAG, LATE_FORCED

    def head_chains(self, default):
        """What the chains of the head's two frames are asked to hold."""
        return dict(step=True), dict(LATE_HEAD_CHAIN[self.seed]) if default else dict(step=True)

    def script(self):
        rng = self.rng
        seeds, head_flag, forced = self.tables()
        default = self.seed in seeds
        a, b, c = (LATE_KINDS[k] for k in (LATE_TRIPLES[self.seed] if default else rng.permutation(5)[:3]))
        flags = head_flag[self.seed] if default else (False, False, (False, True, "async")[int(rng.integers(0, 3))])
        heads = self.head_chains(default)

        def burst(kind, flag):
            if kind == "animated":
                return self.update("animated", "host", flag)
            form = "device" if kind != "transforms" and rng.random() < 0.4 else "host"
            k = "morphed+" if kind == "morphed" and rng.random() < 0.5 else kind
            others = [g for g in self.meshes_for(k) if g != self.x][:2]
            return self.update(k, form, rebuild=flag, meshes=sorted([self.x] + others))
        self.refusals, self.resized = 0, False
        ops = [self.frame(want=heads[0]), burst(a, flags[0]), burst(b, flags[1]), burst(c, flags[2]), self.frame(want=heads[1])]
        units = [tuple(tuple(dict(x) if isinstance(x, dict) else x for x in t) for t in u) for u in forced[self.seed]] if default else []
        room = TAIL_OPS - sum(len(u) for u in units)
        assert room >= 0
        if not any(t[0] == "f" for u in units for t in u):
            units.append((("f", 1, (), bool(rng.random() < 0.4), None),))
            room -= 1
        while room > 0:
            units.append(self.draw_unit(room))
            room -= len(units[-1])
        for k in rng.permutation(len(units)):
            ops += [self.realize(t) for t in units[k]]
        assert len(ops) == OPS
        self.s["ops"] = ops
        return self.s


# ---- the hdr family: variance, variance filter, bloom, quality -----------------------------------------------------------------------
# An hdr script is a late script's scene, size, config, skins, morphs and rig of the same seed with operations of its own, drawn from a
# generator state seeded apart from both other families.  Its operations are the late ones and: variance_reset; the refusals
# vfilter_no_image, variance_bad_config, bloom_bad_levels and quality_bad_ring; and a chain
#     post -> variance -> vfilter -> focus -> bloom -> expose -> quality -> packet -> warp | warp_motion | lens
# whose four new entries are dicts or None:
#   variance  cfg (fovpt_variance_config's five fields), gbuffer "own" (NULL: traced by the call) | "temporal" (fovpt_temporal_gbuffer,
#             only behind a temporal step of this chain), motion (the post step's vectors: exactly when the mask has MOTION), own (the
#             context's image or a caller's), adopt (fovpt_rebuild_state(WAIT | ADOPT) between the step and the call)
#   vfilter   cfg (four iteration counts 0 .. 3, demodulate, three sigmas), input "post" | "accum", variance "own" (NULL) | "given" (the
#             pointer the variance call wrote), out_own; its G-buffer is the variance call's
#   bloom     cfg (fovpt_bloom_config), in_place (out_color == in_color: only on the filter's or the focus step's output, which the
#             chain does not read again), own
#   quality   flags, ring_width, ref "post" | "frame", record_own, classes; the test image is the rgba8 the chain holds there, and the
#             entry exists only where that is not the reference itself
# The restatements of all four stages on a 192 x 128 frame take 0.3 s together (tests/test_app_fuzz_cpu.py measures it), so the BIG
# scripts draw the filter's iteration counts like everybody.
HDR_DEFAULT_SEEDS = range(0, 8)
HDR_SEEDS = range(int(os.environ.get("FOVPT_FUZZHDR_FROM", HDR_DEFAULT_SEEDS.start)), int(os.environ.get("FOVPT_FUZZHDR_TO", HDR_DEFAULT_SEEDS.stop)))
KARIS, GAINS, STATE = 1, 2, 4                            # FOVPT_BLOOM_*
SSIM, PROFILE = 1, 2                                     # FOVPT_QUALITY_*
BLOOM_MAX_LEVELS = 8
HDR_VARIANCE_DEFAULTS = dict(history_cap=16, spatial_below=4, spatial_radius=3, depth_tolerance=0.02, normal_tolerance=0.1)      # variance_ref.MOMENT_DEFAULTS
# what csrc/api_post.hip (variance_check, bloom_check) and csrc/api_view.hip (quality_check) refuse: one step outside each range
VARIANCE_BAD = (("history_cap", 0), ("history_cap", 65), ("spatial_below", -1), ("spatial_radius", 0), ("spatial_radius", 4),
                ("depth_tolerance", 1.5), ("normal_tolerance", 4.5))
BLOOM_BAD_LEVELS = (0, BLOOM_MAX_LEVELS + 1)
QUALITY_BAD_RING = (0, 65537)
ITS = ("iterations_fovea", "iterations_middle", "iterations_periphery", "iterations_uniform")
GAIN_NAMES = ("gain_fovea", "gain_middle", "gain_periphery", "gain_uniform")
NO_MOTION = po.RECONSTRUCT | T_                          # a temporal step that writes no motion vectors
# the kinds and flags of the head's three updates, and the chains of its two frames.  The first chain's bloom reads the exposure
# state before any expose step, the second after the first chain's step (FIXED for seeds 1 and 6); "lit": knee >= threshold, so that
# every pixel with any light passes the bright pass whatever the exposure (checked with bloom_ref on oracle frames of both scenes)
HDR_HEAD_FLAG = [(False, False, "async"), (False, False, True), (False, False, False), (False, False, False),
                 (False, False, True), (False, False, False), (False, False, False), (False, False, False)]
HDR_HEAD_CHAIN = [
    (dict(variance=dict(own=True), bloom=dict(flags=STATE | KARIS, lit=True), expose=("fixed" if s in (1, 6) else "auto")),
     dict(variance=dict(gbuffer="temporal" if s % 2 == 0 else "own", adopt=(s == 0)), vfilter={}, bloom=dict(flags=STATE | (GAINS if s % 4 == 2 else 0), lit=True),
          quality=dict(flags=s % 4), **(dict(last=("lens", 1, False)) if s == 0 else {})))
    for s in range(8)]
HDR_FORCED = [
    # 0: variance_reset; a refused config between two steps of one history; a filter that does nothing; the context's own image
    [(("variance_reset",), ("f", 1, (), False, dict(step=True, variance={}, vfilter=dict(iterations=(0, 0, 0, 0)), quality=dict(flags=0, record_own=False)))),
     (("f", 1, (), False, dict(variance=dict(own=True))), ("x", "variance_bad_config"), ("f", 1, (), False, dict(variance=dict(own=True), vfilter=dict(variance="own"))))],
    # 1: three views in flight with all four stages; temporal_reset, which leaves the moments: first a step with no motion, which
    # reads the history at the pixel itself (a history that wrongly ended would show), then the tracked step whose motion is w = 0
    # everywhere, on moments that are still there
    [(("f", 3, (None, "u"), False, dict(step=True, variance={}, vfilter={}, bloom=dict(lit=True), quality={})),),
     (("temporal_reset",), ("f", 1, (), False, dict(post="none", variance={})), ("f", 1, (), False, dict(step=True, variance={}))),
     (("x", "bloom_bad_levels"),)],
    # 2: expose_reset ahead of a bloom that reads the state; a rebuild between the frame and its chain
    [(("expose_reset",), ("f", 1, (), False, dict(variance={}, bloom=dict(flags=STATE | GAINS, lit=True), expose="auto"))),
     (("f", 1, (), ("vertices", True), dict(step=True, variance=dict(gbuffer="own"))),), (("x", "quality_bad_ring"),)],
    # 3: a resize to the same size, then a step with no motion (with motion the step's w = 0 would hide a history that survived: the
    # temporal history went too); a background build requested between the frame and its chain
    [(("resize", "same"), ("f", 1, (), False, dict(post="none", variance=dict(gbuffer="own")))),
     (("f", 1, (), ("transforms", "async"), dict(step=True, variance=dict(gbuffer="temporal"), quality=dict(flags=SSIM))),)],
    # 4: another size: the filter refused before any variance step there, then accepted; bloom in place, 1 and 8 levels
    [(("resize", "other"), ("f", 1, (), False, dict(variance=False, bloom=dict(levels=1, lit=True))), ("x", "vfilter_no_image"),
      ("f", 1, (), False, dict(step=True, variance=dict(own=True), vfilter=dict(variance="own", out_own=True), bloom=dict(in_place=True, levels=BLOOM_MAX_LEVELS, lit=True))))],
    # 5: set_scene; an adoption between the frame and its chain
    [(("set_scene",), ("f", 1, (), False, dict(post=NO_MOTION, variance={}, bloom=dict(flags=STATE))), ("u", "empty", "host", "async"),
      ("f", 1, (), False, dict(step=True, adopt_first=True, variance=dict(gbuffer="own"))))],
    # 6: no post at all and a post without MOTION; a caller's variance image; the remaining quality flags; focus_reset, which
    # leaves the moments, ahead of a step with no motion
    [(("f", 1, (), False, dict(post="none", variance=dict(own=False), vfilter=dict(variance="given", input="accum"), bloom=dict(in_place=True, levels=1, lit=True),
                               quality=dict(flags=PROFILE, ref="frame"))),),
     (("f", 1, (), False, dict(post=NO_MOTION, variance={}, bloom=dict(flags=STATE), quality=dict(flags=SSIM | PROFILE))),),
     (("focus_reset",), ("f", 1, (), False, dict(post="none", variance={})))],
    # 7: the caller's gaze moved on ahead of everything that reads the frame as rendered
    [(("f", 1, (), False, dict(step=True, moved_on=True, variance={}, vfilter={}, bloom=dict(flags=GAINS | KARIS, lit=True), quality=dict(classes=True, record_own=True))),),
     (("expose_reset",), ("f", 1, (), False, dict(post=NO_MOTION, variance={}, bloom=dict(flags=STATE))))],       # (expose_reset leaves the moments too)
]


class _HdrDraw(_LateDraw):
    def __init__(self, seed):
        super().__init__(seed)                            # (the late script's scene, size, config, skins, morphs and rig)
        self.rng = np.random.default_rng(54000 + seed)
        self.s["hdr"] = True
        self.s["delay_ms"] = 0
        self.rendered = False                             # a frame at this size
        self.var_own = None                               # the size the context's own variance image was written at

    def variance_reset(self):
        return dict(op="variance_reset")

    def resize(self, how=None):
        self.rendered, self.var_own = False, None
        return super().resize(how)

    def refused(self, which):
        rng = self.rng
        if which == "vfilter_no_image":
            assert self.rendered and self.var_own != self.size
            return dict(op="refused", which=which, code=E_NO_FRAME)
        if which == "variance_bad_config":
            name, v = VARIANCE_BAD[int(rng.integers(0, len(VARIANCE_BAD)))]
            return dict(op="refused", which=which, field=name, value=v, code=E_INVALID)
        if which == "bloom_bad_levels":
            return dict(op="refused", which=which, value=int(BLOOM_BAD_LEVELS[int(rng.integers(0, 2))]), code=E_INVALID)
        if which == "quality_bad_ring":
            return dict(op="refused", which=which, value=int(QUALITY_BAD_RING[int(rng.integers(0, 2))]), code=E_INVALID)
        return super().refused(which)

    # ---- the chain
    def hdr_chain(self, c, want):
        """The late chain c with the four new entries; want forces what it names: post ("none" or a mask), expose ("auto", "fixed",
        None), variance / vfilter / bloom / quality (False: absent; a dict: present, with these entries)."""
        rng = self.rng
        if "post" in want:
            c["post"] = None if want["post"] == "none" else int(want["post"])
        if "expose" in want:
            c["expose"] = None if want["expose"] is None else dict(self.expose_config(), mode=AUTO if want["expose"] == "auto" else FIXED)
        post = c["post"]
        has_t, has_m = post is not None and bool(post & T_), post is not None and bool(post & M_)
        present = lambda name, p: want.get(name) is not False and (want.get(name) is not None or rng.random() < p)
        src = origin = "frame" if post is None else "post"

        v = None
        if present("variance", 0.7):
            cap = int(rng.choice([2, 3, 16]))
            below = int(rng.choice([0, 2, 4] if cap > 2 else [0, 2]))       # (spatial_below above history_cap + 1 is refused)
            cfg = dict(history_cap=cap, spatial_below=below, spatial_radius=int(rng.integers(1, 4)),
                       depth_tolerance=float(F(rng.uniform(0.005, 0.2))), normal_tolerance=float(F(rng.uniform(0.0, 1.0))))
            v = dict(cfg=cfg, gbuffer="temporal" if has_t and rng.random() < 0.5 else "own", motion=has_m, own=bool(rng.random() < 0.6), adopt=False)
            for k, x in (want.get("variance") or {}).items():
                (cfg if k in cfg else v)[k] = x
            assert v["gbuffer"] == "own" or has_t
            if v["own"]:
                self.var_own = self.size
        f = None
        if v is not None and present("vfilter", 0.7):
            cfg = dict(zip(ITS, (int(x) for x in rng.integers(0, 4, 4))), demodulate=int(rng.integers(0, 2)),
                       luminance_sigma=float(F(4.0 * np.exp2(rng.uniform(-1, 1)))), normal_sigma=float(F(0.5 * np.exp2(rng.uniform(-1, 1)))),
                       depth_sigma=float(F(0.05 * np.exp2(rng.uniform(-1, 1)))))
            f = dict(cfg=cfg, input="post" if post is not None and rng.random() < 0.6 else "accum",
                     variance="own" if v["own"] and rng.random() < 0.5 else "given", out_own=bool(rng.random() < 0.5))
            for k, x in (want.get("vfilter") or {}).items():
                if k == "iterations":
                    cfg.update(zip(ITS, x))
                else:
                    (cfg if k in cfg else f)[k] = x
            assert (f["input"] == "accum" or post is not None) and (f["variance"] == "given" or v["own"])
            src = origin = "vfilter"
        if c["focus"] is not None:
            src = origin = "focus"
        b = None
        if present("bloom", 0.6):
            pick = lambda: float(F((0.0, 0.125, 1.0, rng.uniform(0, 1))[int(rng.integers(0, 4))]))
            cfg = dict(flags=int(rng.integers(0, 8)), levels=int(rng.integers(1, BLOOM_MAX_LEVELS + 1)), threshold=float(F(np.exp2(rng.uniform(-6, 1)))),
                       knee=float(F(np.exp2(rng.uniform(-6, 1)))) if rng.random() < 0.8 else 0.0, exposure=float(F(np.exp2(rng.uniform(0, 6)))),
                       intensity=float(F(rng.uniform(0, 0.5))), spread=float(F(rng.uniform(0, 1))), **{g: pick() for g in GAIN_NAMES})
            b = dict(cfg=cfg, in_place=bool(src in ("vfilter", "focus") and rng.random() < 0.4), own=bool(rng.random() < 0.5))
            wb = dict(want.get("bloom") or {})
            lit = wb.pop("lit", False)
            for k, x in wb.items():
                (cfg if k in cfg else b)[k] = x
            if lit:
                cfg["knee"] = max(cfg["knee"], cfg["threshold"])
                cfg.update(gain_fovea=1.0, gain_uniform=1.0)
            assert not b["in_place"] or src in ("vfilter", "focus")
            origin = "bloom"
        if c["expose"] is not None:
            origin = "expose"
        q = None
        refs = [x for x in (("post",) if post is not None else ()) + ("frame",) if x != origin]
        if refs and present("quality", 0.6):
            q = dict(flags=int(rng.integers(0, 4)), ring_width=int(rng.choice([1, 3, 16])), ref=refs[int(rng.integers(0, len(refs)))],
                     record_own=bool(rng.random() < 0.5), classes=bool(rng.random() < 0.5))
            q.update(want.get("quality") or {})
            assert q["ref"] in refs
        c.update(variance=v, vfilter=f, bloom=b, quality=q)
        return c

    def frame(self, n=1, between=(), pre_chain=False, want=None):
        want = dict(want) if isinstance(want, dict) else dict(step=True) if want in ("step", "step+packet") else {}
        flag = False
        if isinstance(pre_chain, tuple):
            pre_chain, flag = pre_chain
        late = {k: want[k] for k in ("step", "focus", "last", "codec", "adopt_first") if k in want}
        if "post" in want and not (want["post"] != "none" and want["post"] & T_ and want["post"] & M_):
            late.update(focus=None, last=(None,))         # (neither stage has a tracked step to lean on)
        if (want.get("variance") or {}).get("adopt"):
            late.setdefault("last", (None,))              # (a warp_motion on the step's G-buffer would be refused: the late family's case)
        stepped = self.stepped
        op = super().frame(n, between, pre_chain, late)
        if flag:
            op["pre_chain"]["rebuild"] = flag
        if want.get("moved_on") and op["moved_on"] is None:
            w, h = self.size
            op["moved_on"] = dict(gaze=(int(self.rng.integers(-10, w + 11)), int(self.rng.integers(-10, h + 11))), subframe_index=int(self.rng.integers(4, 9)))
        self.rendered = True
        op["chain"] = self.hdr_chain(op["chain"], want)
        post = op["chain"]["post"]
        self.stepped = stepped or (post is not None and bool(post & T_))
        return op

    def draw_unit(self, room):
        rng = self.rng
        while True:
            u = rng.random()
            if u < 0.45:
                unit = super().draw_unit(room)
            elif u < 0.70:
                n = int(rng.integers(1, 4))
                unit = (("f", n, (None,) * (n - 1), bool(rng.random() < 0.3), None),)
            elif u < 0.80:
                unit = ((("variance_reset",),), (("variance_reset",), ("f", 1, (), False, dict(variance={}))))[int(rng.integers(0, 2))]
            elif u < 0.90:
                unit = ((("x", "bloom_bad_levels"),), (("x", "quality_bad_ring"),),
                        (("f", 1, (), False, dict(variance={})), ("x", "variance_bad_config"), ("f", 1, (), False, dict(variance={}))),
                        (("resize", "other"), ("f", 1, (), False, dict(variance=False)), ("x", "vfilter_no_image")))[int(rng.integers(0, 4))]
            else:
                unit = (("expose_reset",), ("f", 1, (), False, dict(bloom=dict(flags=STATE))))
            if len(unit) <= room:
                return unit

    def realize(self, t):
        if t[0] == "x" and t[1] == "vfilter_no_image" and self.refusals < MAX_REFUSED and not (self.rendered and self.var_own != self.size):
            return self.temporal_reset()                  # (nothing to refuse here: something harmless in its place)
        return super().realize(t)

    def tables(self):
        return HDR_DEFAULT_SEEDS, HDR_HEAD_FLAG, HDR_FORCED

    def head_chains(self, default):
        first, second = HDR_HEAD_CHAIN[self.seed] if default else (dict(variance={}), dict(variance={}))
        return dict(first, step=True), dict(second, step=True)


def script(seed, late=False, hdr=False):
    return (_HdrDraw if hdr else _LateDraw if late else _Draw)(int(seed)).script()
