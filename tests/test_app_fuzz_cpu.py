"""tests/app_fuzz.py without a GPU: the scripts are a pure function of the seed, the default seeds reach every operation and every
situation the sweep of tests/test_app_fuzz_gpu.py is there for, every pose drawn as valid passes the overflow rule of its kind
and every pose drawn as refused does not, and a dry run of the positions (tests/app_model.dry_run) stays finite.

The old scripts are pinned by a digest (seeds 0 .. 31).  The late family (af.script(seed, late=True)) gets the same five tests over
af.LATE_DEFAULT_SEEDS through walk_late(), which follows the rig, the tracking, the interval and the background build on its own:
  operations   LATE_OPERATIONS: update_animated with no flag, REBUILD and REBUILD_ASYNC; REBUILD_ASYNC on the other four kinds and
               with no entries; rebuild_state with 0, WAIT, ADOPT and WAIT | ADOPT; focus FIXED and AUTO, on the temporal G-buffer and
               on its own trace; focus_reset; warp; warp_motion both ways and with every advance; the three lens filters with and
               without a camera; coded packets with a BC1, a raw and a BY_FILL pass; the refusals no_rig, clip_range,
               async_with_rebuild and warp_motion_stale; the four kinds of binding, STEP and LINEAR channels of all four paths, the
               four cases of the sample rule and the three branches of the rotation rule
  situations   LATE_SITUATIONS: the eight ordered pairs of "animated" with another kind on one mesh in one tracked interval;
               set_skins, set_morphs and set_scene each followed by a refused update_animated, a new set_rig and an accepted one; a
               request while a build is in flight; adoption by a later update after WAIT, by rebuild_state(ADOPT), between two
               frames in flight, inside a tracked interval, and with an update between snapshot and adoption; a build ended by
               set_scene and one ended by REBUILD; warp_motion with a moved mesh, when nothing moved and after a step that did not
               know the motion; refused after an update, refused with a G-buffer traced before an adoption and accepted again after
               a fresh trace; focus AUTO across a resize; a coded packet on the first frame of another size, on a frame of partial
               blocks and on the (3, 50) frame (refused with FOVPT_E_INVALID: a packet that would not pass fovpt_packet_check)
  caps         ten operations, at most 2 refused calls, at least 3 chained frame groups, a new operation in every default script
LATE_OWN names what each default seed's forced units are there for, seed by seed: taking any one unit out of af.LATE_FORCED makes
test_each_late_default_seed_holds_its_own_units fail (tried for all of them).

The build's state in walk_late is "no", "yes" or "maybe": an update that enqueues something while a build is in flight adopts the
result if the builder has finished, which no script can know without rebuild_state(WAIT) before it; the model reads which one
happened (tests/app_model.LateModel), the walker counts a situation only where it is certain -- with one exception that cannot be
made certain: "an update between snapshot and adoption" is counted where updates follow a request without a wait and
rebuild_state(WAIT | ADOPT) follows them; whether the adoption then finds a snapshot older than the positions depends on whether
those updates met the build still running (any of them that met it READY adopted it itself, with nothing in between).

The late scripts are pinned by a digest as well (seeds 0 .. 31, computed before the hdr family was added).  The hdr family
(af.script(seed, hdr=True)) gets the same five tests and a digest through walk_hdr(), which follows the tracking and the interval,
the events since the last variance step, the moment history, the context's variance image, the exposure state's last event and
the background build, and checks every new chain entry against the ranges the library validates:
  operations   HDR_OPERATIONS: the four stages, variance_reset, the four refusals, both G-buffers, both images, both filter inputs
               and outputs, both quality references
  situations   HDR_SITUATIONS, listed in test_the_hdr_default_seeds_reach_every_situation
  own units    HDR_OWN: what each default seed's forced units and head chains are there for
test_the_restatements_of_an_hdr_chain_stay_finite_and_quick runs the four restatements without a renderer on a synthetic frame for
every size and chain config of the default scripts: moments twice, the filter, bloom and quality of one chain take 0.34 s at
192 x 128 on the CPU (0.04 s at 64 x 45, 0.09 s at 96 x 64), beside post_ref.post's 0.21 s there, so the 192 x 128 scripts draw the
filter's iteration counts like every other size."""
import hashlib

import numpy as np
import pytest

import app_fuzz as af
import app_model as am
import morph_ref as mr
import post_ref as po
import rig_ref as rg
import skin_ref as sk
import transform_ref as tf

KINDS = af.KINDS
F = np.float32


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a, key=str) == sorted(b, key=str) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return type(a) is type(b) and a == b


def _accepted(model, kind, k, pose, skins, morphs):
    rest = model.meshes[k].vertex
    if kind == "vertices":
        return bool(np.isfinite(pose).all()) and pose.shape == rest.shape
    if kind == "transforms":
        return tf.accepted(rest, pose)
    if kind == "skinned":
        return sk.palette(pose).shape[0] == skins[k][2] and sk.accepted(rest, skins[k][1], pose)
    w, pal = pose if isinstance(pose, tuple) else (pose, None)
    if len(w) != len(morphs[k]) or (pal is not None and sk.palette(pal).shape[0] != skins[k][2]):
        return False
    return mr.accepted(rest, morphs[k], w, skins[k][1] if pal is not None else None, pal)


def walk(s, model):
    """The features of one script -> (set of names, refused operations, frames with a chain)."""
    seen, refused, chained = set(), 0, 0
    skins, morphs = dict(s["skins"]), dict(s["morphs"])
    interval = {}                                         # mesh -> the kinds that moved it since the previous temporal step
    steps, resized, rebuilt = 0, False, False             # tracked temporal steps since the scene was set; events since the last one
    new_size = False                                      # a resize to another size, no frame since
    ops, size = s["ops"], s["size"]

    def update(u, where):
        nonlocal rebuilt
        plus = any(isinstance(p, tuple) for p in u["poses"].values())
        seen.add("update:%s%s:%s" % (u["kind"], "+" if plus else "", "device" if u["device"] else "host"))
        if not u["poses"]:
            seen.add("update:empty")
        if u["rebuild"]:
            seen.add("rebuild:" + u["kind"])
            rebuilt = rebuilt or steps > 0
        if len(u["poses"]) > af.GATHER_BATCH:
            seen.add("more than one batch")
        if len(u["poses"]) < len(model.meshes):
            seen.add("a subset of the meshes")
        for k, p in u["poses"].items():
            assert _accepted(model, u["kind"], k, p, skins, morphs), (s["seed"], u["kind"], k)
            for a in interval.get(k, []):
                if a != u["kind"] and steps > 0:
                    seen.add("pair:%s>%s" % (a, u["kind"]))
            interval.setdefault(k, []).append(u["kind"])
        seen.add("update " + where)

    def refuse(x, where):
        nonlocal refused
        refused += 1
        seen.add("refused:" + x["which"])
        seen.add("refused " + where)
        if x["which"] == "overflow":
            assert not _accepted(model, x["kind"], x["bad"], x["poses"][x["bad"]], skins, morphs), (s["seed"], x["kind"])
            assert all(_accepted(model, x["kind"], k, p, skins, morphs) for k, p in x["poses"].items() if k != x["bad"])
        elif x["which"] == "mesh_range":
            assert not 0 <= x["bad"] < len(model.meshes)
        elif x["which"] == "no_skin":
            assert x["bad"] not in skins

    for i, op in enumerate(ops):
        kind = op["op"]
        if kind == "update":
            update(op, "alone")
            before = [o["op"] for o in ops[max(0, i - 2):i]]
            if op["poses"] and (before[-1:] == ["resize"] or (before == ["resize", "refused"] and ops[i - 1]["which"] == "no_frame")):
                seen.add("a pose right after a resize")
        elif kind == "refused":
            refuse(op, "alone")
            if op["which"] == "no_frame":
                assert ops[i - 1]["op"] == "resize"
        elif kind in ("set_skins", "set_morphs"):
            seen.add(kind)
            new = op["skins" if kind == "set_skins" else "morphs"]
            have = skins if kind == "set_skins" else morphs
            for k, v in new.items():
                seen.add("%s %s" % (kind, "removes" if v is None else "replaces" if k in have else "adds"))
            prev = ops[i - 1]
            if prev["op"] == "update" and prev["poses"] and prev["kind"] == ("skinned" if kind == "set_skins" else "morphed"):
                seen.add(kind + " directly after a pose of the old layout")
            am.register(have, new)
            nxt = ops[i + 1] if i + 1 < len(ops) else None
            if kind == "set_skins" and nxt and nxt["op"] == "update" and nxt["kind"] == "skinned" and not nxt["device"] and sorted(nxt["poses"]) == sorted(skins):
                seen.add("every skin posed from the host directly after set_skins")
        elif kind == "frame":
            n = len(op["views"])
            assert 1 <= n <= 3 and len(op["between"]) == n - 1
            seen.add("frames:%d" % n)
            seen.add("render" if op["sync"] else "render_async")
            for b in op["between"]:
                if b is not None:
                    (update if b["op"] == "update" else refuse)(b, "between two frames in flight")
            c = op["chain"]
            if op["pre_chain"] is not None:
                assert c["post"] is not None or c["expose"] is not None or c["packet"]
                update(op["pre_chain"], "between a render and its post chain")
            if c["post"] is not None or c["expose"] is not None or c["packet"]:
                chained += 1
                if op["moved_on"] is not None:
                    seen.add("the chain runs after the caller's gaze moved on")
            if c["post"] is not None:
                assert c["post"] in po.VALID_STAGES
                seen.add("post")
                seen.add("post:%d" % c["post"])
            if c["expose"] is not None:
                seen.add("expose on " + ("post" if c["post"] is not None else "accum"))
            if c["packet"]:
                seen.add("packet on " + ("expose" if c["expose"] is not None else "post" if c["post"] is not None else "the frame"))
            tracked = c["post"] is not None and c["post"] & po.TEMPORAL and c["post"] & po.MOTION
            if new_size and tracked and c["packet"] and min(size) >= 4:
                seen.add("a tracked step and a packet on the first frame of another size")
            new_size = False
            if c["post"] is not None and c["post"] & po.TEMPORAL and not tracked and steps == 0:
                interval.clear()                          # (a plain step before tracking began: an interval nobody tracks)
            if c["post"] is not None and c["post"] & po.TEMPORAL and (tracked or steps > 0):
                if steps > 0 and resized:
                    seen.add("a resize between two temporal steps")
                if steps > 0 and rebuilt:
                    seen.add("a rebuild inside an interval")
                steps += 1
                resized = rebuilt = False
                interval.clear()
        elif kind == "resize":
            assert op["size"] in af.SIZES or op["size"] == s["size"]
            seen.add("resize")
            seen.add("resize to the same size" if op["size"] == size else "resize to another size")
            new_size = op["size"] != size
            size = op["size"]
            resized = True
        elif kind == "set_scene":
            seen.add("set_scene")
            skins, morphs = {}, {}
            interval.clear()
            steps, resized, rebuilt = 0, False, False         # (tracking is off until the next step with motion)
        else:
            assert kind in ("temporal_reset", "expose_reset"), kind
            seen.add(kind)
    return seen, refused, chained


@pytest.fixture(scope="module")
def walked():
    out = {}
    for seed in af.DEFAULT_SEEDS:
        s = af.script(seed)
        model, _ = af.scene_of(s)
        out[seed] = (s, model, walk(s, model))
    return out


def test_a_script_is_a_pure_function_of_the_seed():
    for seed in (0, 2, 5):
        assert _same(af.script(seed), af.script(seed))
    orders = {tuple(o["op"] for o in af.script(seed)["ops"][5:]) for seed in range(8, 32) if seed % 8 not in (2, 5)}
    assert len(orders) >= 12, len(orders)                            # the order of the operations is drawn, not read from a table


def test_every_script_does_something(walked):
    """The cap: ten operations, at most 2 of them refused calls, at least 3 frames followed by at least one post-chain stage:
    for the default seeds and, the scripts being drawn, for the next 24 (whose poses walk() checks against the overflow rules
    of their kinds as well)."""
    more = {}
    for seed in range(8, 32):
        s = af.script(seed)
        more[seed] = (s, None, walk(s, af.scene_of(s)[0]))
    for seed, (s, _, (_, refused, chained)) in list(walked.items()) + list(more.items()):
        assert len(s["ops"]) == af.OPS == 10
        assert refused <= 2 and chained >= 3, (seed, refused, chained)


def test_the_default_seeds_reach_every_operation(walked):
    seen = set().union(*(w[2][0] for w in walked.values()))
    want = ["update:vertices:host", "update:vertices:device", "update:transforms:host", "update:skinned:host", "update:skinned:device",
            "update:morphed:host", "update:morphed:device", "update:morphed+:host", "update:morphed+:device", "update:empty",
            "a subset of the meshes", "set_skins", "set_morphs", "render", "render_async", "frames:1", "frames:2", "frames:3",
            "post", "expose on post", "expose on accum", "packet on expose", "packet on post", "packet on the frame",
            "resize", "resize to the same size", "resize to another size", "set_scene", "temporal_reset", "expose_reset",
            "refused:overflow", "refused:mesh_range", "refused:no_skin", "refused:no_frame"]
    want += ["rebuild:" + k for k in KINDS]
    want += ["%s %s" % (a, b) for a in ("set_skins", "set_morphs") for b in ("replaces", "removes", "adds")]
    missing = [w for w in want if w not in seen]
    assert not missing, missing
    assert len({x for x in seen if x.startswith("post:")}) >= 5        # several stage masks, the fused ones among them
    assert any(int(x[5:]) & po.RECONSTRUCT and int(x[5:]) & po.TEMPORAL for x in seen if x.startswith("post:"))


def test_the_default_seeds_reach_every_situation(walked):
    seen = set().union(*(w[2][0] for w in walked.values()))
    want = ["pair:%s>%s" % (a, b) for a in KINDS for b in KINDS if a != b]
    want += ["a rebuild inside an interval", "update between a render and its post chain", "update between two frames in flight",
             "set_skins directly after a pose of the old layout", "set_morphs directly after a pose of the old layout",
             "a resize between two temporal steps", "refused between two frames in flight", "more than one batch",
             "every skin posed from the host directly after set_skins", "a pose right after a resize",
             "a tracked step and a packet on the first frame of another size", "the chain runs after the caller's gaze moved on"]
    missing = [w for w in want if w not in seen]
    assert not missing, missing


def test_shapes_and_budgets(walked):
    scenes_seen, fif, chains = set(), 0, 0
    for seed, (s, model, _) in walked.items():
        c, (w, h) = s["config"], s["size"]
        scenes_seen.add(s["scene"][0])
        assert max(c["spp"]) <= 4 and 1 <= c["max_depth"] <= 3
        if s["scene"][0] == "atrium":
            assert 500 <= s["scene"][1] <= 2000 and len(model.meshes) > af.GATHER_BATCH
        fif += c["frames_in_flight"] == 2
        if c["chains_per_frame"] == 2:
            chains += 1
            assert (w, h) == af.BIG and not c["uniform"]
            assert np.pi * min(c["r_inner"], 60) ** 2 * 0.9 * c["spp"][2] >= 16384          # the fovea alone, on a 192 x 128 frame
        else:
            assert w <= 130 and h <= 90
    assert scenes_seen == {"cornell", "atrium"} and fif == 2 and chains == 2      # one seed in four each
    assert any(w < 4 for w, h in af.SIZES) and any(w % 64 == 63 and h % 4 for w, h in af.SIZES) and any(w % 64 == 1 and h % 4 for w, h in af.SIZES)


def test_dry_run_keeps_every_position_finite(walked):
    for seed, (s, model, _) in walked.items():
        vtx = am.dry_run(s, model)
        assert np.isfinite(vtx).all() and vtx.shape[0] == sum(m.vertex.shape[0] for m in model.meshes)
        if not any(o["op"] == "set_scene" for o in s["ops"]):
            assert not np.array_equal(vtx, np.concatenate([m.vertex for m in model.meshes]))          # (it did move)


# ---- the old scripts are pinned ------------------------------------------------------------------------------------------------
def _feed(h, x):
    """The canonical serialisation of a script, fed to a hash: containers with their kind and length, dict entries in the order
    of their keys' str, arrays with dtype, shape and bytes, everything else with its type's name and its repr."""
    if isinstance(x, dict):
        h.update(b"d%d;" % len(x))
        for k in sorted(x, key=str):
            h.update(repr(k).encode() + b":")
            _feed(h, x[k])
    elif isinstance(x, (list, tuple)):
        h.update((b"l%d;" if isinstance(x, list) else b"t%d;") % len(x))
        for y in x:
            _feed(h, y)
    elif isinstance(x, np.ndarray):
        h.update(b"a" + x.dtype.str.encode() + repr(x.shape).encode())
        h.update(np.ascontiguousarray(x).tobytes())
    else:
        h.update(type(x).__name__.encode() + b"=" + repr(x).encode() + b";")


# sha256 over the scripts of seeds 0 .. 31, computed with the generator as it was before the late family was added
OLD_SCRIPTS_DIGEST = "4030e928ee20975c8dae17837f2ead653f192b3b0d8b64a9957184229d567c48"


def test_the_old_scripts_are_what_they_were():
    h = hashlib.sha256()
    for seed in range(32):
        _feed(h, af.script(seed))
    assert h.hexdigest() == OLD_SCRIPTS_DIGEST
    assert not any("late" in af.script(seed) or "rig" in af.script(seed) for seed in (0, 9))


# ---- the late family ---------------------------------------------------------------------------------------------------------------
NEW_OPS = ("update:animated", "async:", "rebuild_state:", "focus:", "focus_reset", "warp", "lens:", "coded:", "set_rig",
           "refused:no_rig", "refused:clip_range", "refused:async_with_rebuild", "refused:warp_motion_stale")


def _levels(parent):
    d = np.zeros(len(parent), np.int64)
    for i, p in enumerate(parent):
        d[i] = 0 if p < 0 else d[p] + 1
    return int(d.max()) + 1


def _rig_features(seen, rig, nmesh, skins, morphs):
    assert rg.accepted(rig, nmesh, {k: v[2] for k, v in skins.items()}, {k: len(v) for k, v in morphs.items()})
    assert _levels(rig["parent"]) >= 3 and len(rig["parent"]) <= 48
    for b in rig["bindings"]:
        joints, morphed = b.get("joint_nodes") is not None, b["mesh"] in morphs
        seen.add("binding:" + ("morph+skin" if joints and morphed else "skinned" if joints else "morph" if morphed else "rigid"))
    for ch in rig["clips"][0]:
        seen.add("channel:%d:%s" % (ch["path"], "step" if ch["interpolation"] == rg.STEP else "linear"))


def _sample_features(seen, rig, clip, T):
    """Which cases of the header's sample rule and of its rotation rule a pose at T takes."""
    for ch in rig["clips"][clip]:
        t = np.asarray(ch["times"], F)
        k, u = rg.locate(t, T)
        seen.add("sample:" + ("before" if F(T) <= t[0] else "after" if F(T) >= t[-1] else "key" if F(T) in t else "between"))
        if u is not None and ch["path"] == rg.ROTATION and ch["interpolation"] == rg.LINEAR:
            a, b = ch["values"][k], ch["values"][k + 1]
            d = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]
            if d < 0:
                seen.add("slerp:flip")
            seen.add("slerp:lerp" if abs(d) > rg.SLERP_LINEAR_ABOVE else "slerp:slerp")


def walk_late(s, model, oracle):
    """walk() for a late script -> (set of names, refused operations, frames with a chain).  It follows on its own what the
    generator must have followed to draw valid operations: the rig, the tracking, the interval and the background build, whose
    state is "no", "yes" (in flight for certain) or "maybe" (an update that enqueues something ran since the request without a
    wait before it: it has adopted the result or it has not), with `ready` once a wait has run."""
    seen, refused, chained = set(), 0, 0
    nmesh = len(model.meshes)
    skins, morphs, rig = dict(s["skins"]), dict(s["morphs"]), s["rig"]
    _rig_features(seen, rig, nmesh, skins, morphs)
    interval, last_interval = {}, {}
    tracking = untracked = stepped = known = False        # known: the last step knew its interval's motion
    steps, moved_since_step, open_adoption = 0, False, False
    build = dict(flight="no", ready=False, since=0)
    auto_steps, resized_since_auto, new_size = 0, False, False
    ops, size = s["ops"], s["size"]

    def adoption(how, where):
        nonlocal open_adoption
        seen.add("an adopting update between two frames in flight" if where == "between" else "adoption by " + how)
        if build["since"] >= 1:
            seen.add("an update between snapshot and adoption")
        open_adoption = open_adoption or (stepped and tracking)
        build.update(flight="no", ready=False, since=0)

    def update(u, where):
        nonlocal untracked, moved_since_step
        kind, flag = u["kind"], u["rebuild"]
        animated = kind == "animated"
        assert flag in (False, True, "async") and (animated or isinstance(u["poses"], dict))
        moves = animated or bool(u["poses"])
        entry = build["flight"]                           # a request looks at the state the call finds
        if flag is True:
            seen.add("rebuild:" + kind)
            if build["flight"] == "yes":
                seen.add("a build ended by REBUILD")
            build.update(flight="no", ready=False, since=0)
        elif moves and build["flight"] != "no":
            if build["flight"] == "yes" and build["ready"]:
                adoption("a later update after WAIT", where)
            else:
                build.update(flight="maybe", since=build["since"] + 1)
        if flag == "async":
            seen.add("async:" + (kind if moves else "empty"))
            if entry == "yes":
                seen.add("a request while a build is in flight")      # (counted, and nothing started, whatever the call adopts)
            elif entry == "no":
                build.update(flight="yes", ready=False, since=0)
            else:                                         # in flight and ignored, or idle and started
                build.update(flight="maybe" if moves else "yes", ready=False, since=0)
        if animated:
            assert rig is not None and 0 <= u["poses"]["clip"] < len(rig["clips"])
            seen.add("update:animated" + (":rebuild" if flag is True else ":async" if flag else ":refit"))
            _sample_features(seen, rig, u["poses"]["clip"], u["poses"]["time"])
            new = rg.restate(oracle, model, rig, u["poses"]["clip"], u["poses"]["time"], skins, morphs)
            assert sorted(new) == sorted(b["mesh"] for b in rig["bindings"]) and all(np.isfinite(v).all() for v in new.values())
            meshes = sorted(new)
        else:
            for k, p in u["poses"].items():
                assert _accepted(model, kind, k, p, skins, morphs), (s["seed"], kind, k)
            meshes = sorted(u["poses"])
        for k in meshes:
            for a in interval.get(k, []):
                if a != kind and steps > 0 and "animated" in (a, kind):
                    seen.add("pair:%s>%s" % (a, kind))
            interval.setdefault(k, []).append(kind)
        if meshes:
            moved_since_step = True
            untracked = untracked or not tracking
        seen.add("update " + where)

    def refuse(x, where):
        nonlocal refused
        refused += 1
        seen.add("refused:" + x["which"])
        if x["which"] == "no_rig":
            assert rig is None
        elif x["which"] == "clip_range":
            assert rig is not None and not 0 <= x["clip"] < len(rig["clips"])
        elif x["which"] == "async_with_rebuild":
            assert x["kind"] == "vertices" or rig is not None
        elif x["which"] == "warp_motion_stale":
            assert stepped and tracking and moved_since_step and where == "alone"
        elif x["which"] == "overflow":
            assert not _accepted(model, x["kind"], x["bad"], x["poses"][x["bad"]], skins, morphs)
        elif x["which"] == "no_skin":
            assert x["bad"] not in skins

    for i, op in enumerate(ops):
        kind = op["op"]
        if kind == "update":
            update(op, "alone")
        elif kind == "refused":
            refuse(op, "alone")
            if op["which"] in ("no_rig",) and i + 2 < len(ops) and ops[i - 1]["op"] in ("set_skins", "set_morphs", "set_scene") and ops[i + 1]["op"] == "set_rig":
                nxt = [u for u, _ in am.updates_of(ops[i + 2])]
                if nxt and nxt[-1]["kind"] == "animated" or (ops[i + 2]["op"] == "frame" and ops[i + 2]["pre_chain"] and ops[i + 2]["pre_chain"]["kind"] == "animated"):
                    seen.add("%s, a refused update_animated, set_rig and an accepted one" % ops[i - 1]["op"])
        elif kind in ("set_skins", "set_morphs"):
            seen.add(kind)
            am.register(skins if kind == "set_skins" else morphs, op["skins" if kind == "set_skins" else "morphs"])
            rig = None
        elif kind == "set_rig":
            seen.add("set_rig")
            rig = op["rig"]
            _rig_features(set(), rig, nmesh, skins, morphs)
        elif kind == "rebuild_state":
            seen.add("rebuild_state:%d" % (op["wait"] + 2 * op["adopt"]))
            if op["wait"] and build["flight"] != "no":
                build["ready"] = True
            if op["adopt"] and build["flight"] == "yes" and build["ready"]:
                adoption("rebuild_state(ADOPT)", "alone")
            elif op["adopt"] and build["flight"] != "no":
                build.update(flight="no" if build["ready"] else "maybe")
        elif kind == "focus_reset":
            seen.add("focus_reset")
            auto_steps = 0
        elif kind == "frame":
            n = len(op["views"])
            assert 1 <= n <= 3 and len(op["between"]) == n - 1
            seen.add("frames:%d" % n)
            for b in op["between"]:
                if b is not None:
                    (update if b["op"] == "update" else refuse)(b, "between")
            if op["adopt_first"]:
                if build["flight"] != "no":
                    if build["since"] >= 1:                   # (set up, not certain: with "maybe" an update may have adopted itself)
                        seen.add("an update between snapshot and adoption")
                    if build["flight"] == "yes":
                        build["ready"] = True
                        adoption("rebuild_state(ADOPT)", "alone")
                    build.update(flight="no", ready=False, since=0)
            c = op["chain"]
            if op["pre_chain"] is not None:
                update(op["pre_chain"], "between a render and its post chain")
            chained += any(c[k] is not None for k in ("post", "expose", "focus", "last")) or c["packet"]
            post = c["post"]
            temporal = post is not None and bool(post & po.TEMPORAL)
            if post is not None:
                assert post in po.VALID_STAGES
                seen.add("post")
            if temporal:
                if post & po.MOTION:
                    tracking = True
                known = not untracked
                if tracking and stepped and open_adoption:
                    seen.add("an adoption inside a tracked interval")
                if tracking:
                    steps += 1
                last_interval, interval = dict(interval), {}
                untracked = moved_since_step = open_adoption = False
                stepped = True
            f = c["focus"]
            if f is not None:
                assert f["gbuffer"] == "own" or temporal
                seen.add("focus:" + ("auto" if f["mode"] == af.AUTO else "fixed"))
                seen.add("focus on " + ("the temporal G-buffer" if f["gbuffer"] == "temporal" else "its own trace"))
                if f["mode"] == af.AUTO:
                    if auto_steps and resized_since_auto:
                        seen.add("focus AUTO across a resize")
                    auto_steps, resized_since_auto = auto_steps + 1, False
            if c["packet"] and c["codec"] is not None:
                assert len(c["codec"]) == 3 and all(k in (af.RAW, af.BC1, af.BY_FILL) for k in c["codec"])
                for k in c["codec"]:
                    seen.add("coded:" + {af.RAW: "raw", af.BC1: "bc1", af.BY_FILL: "by_fill"}[k])
                if new_size and min(size) >= 4:
                    seen.add("a coded packet on the first frame of another size")
                if size[0] % 4 and size[1] % 4 and min(size) >= 4:
                    seen.add("a coded packet on a frame of partial blocks")
                if tuple(size) == (3, 50):
                    seen.add("a coded packet on the (3, 50) frame")
            elif c["packet"]:
                seen.add("packet:raw")
            new_size = False
            la = c["last"]
            if la is not None and la["stage"] == "lens":
                assert la["filter"] in (0, 1, 2) and len(la["chroma"]) == 3
                seen.add("lens:%d:%s" % (la["filter"], "camera" if la["to"] is not None else "no camera"))
            elif la is not None:
                assert la["images"] in (1, 2, 3) and 0 <= la["fill_radius"] <= 3 and la["to"][0] in ("slide", "turn", "dolly")
                seen.add("images:%d" % la["images"])
                seen.add(la["stage"])
                if la["stage"] == "warp_motion":
                    assert temporal and tracking and la["advance"] in af.ADVANCES and not moved_since_step
                    seen.add("warp_motion on " + ("the temporal G-buffer" if la["gbuffer"] == "temporal" else "its own trace"))
                    seen.add("advance:%g" % la["advance"])
                    if not known:
                        seen.add("warp_motion after a step that did not know the motion")
                    elif not last_interval:
                        seen.add("warp_motion when nothing moved")
                    elif la["advance"] > 0:
                        seen.add("warp_motion with a moved mesh")
                    if la["adopt"]:
                        assert la["gbuffer"] == "temporal" and build["flight"] == "yes", (s["seed"], build)
                        seen.add("a stale G-buffer refused after an adoption, accepted after a fresh trace")
                        build["ready"] = True
                        adoption("rebuild_state(ADOPT)", "alone")
        elif kind == "resize":
            seen.add("resize")
            new_size = tuple(op["size"]) != tuple(size)
            size = op["size"]
            stepped, open_adoption = False, False
            interval.clear()
            resized_since_auto = True
        elif kind == "set_scene":
            seen.add("set_scene")
            if build["flight"] == "yes":
                seen.add("a build ended by set_scene")
            build.update(flight="no", ready=False, since=0)
            skins, morphs, rig = {}, {}, None
            interval.clear()
            tracking = untracked = stepped = moved_since_step = open_adoption = False
            steps, auto_steps = 0, 0
        else:
            assert kind in ("temporal_reset", "expose_reset"), kind
            seen.add(kind)
            if kind == "temporal_reset":
                stepped, open_adoption = False, False
    return seen, refused, chained


LATE_OPERATIONS = (["update:animated:refit", "update:animated:rebuild", "update:animated:async", "async:vertices", "async:transforms", "async:skinned",
                    "async:morphed", "async:empty", "rebuild_state:0", "rebuild_state:1", "rebuild_state:2", "rebuild_state:3",
                    "focus:fixed", "focus:auto", "focus on the temporal G-buffer", "focus on its own trace", "focus_reset", "warp",
                    "warp_motion on its own trace", "warp_motion on the temporal G-buffer", "images:1", "images:2", "coded:bc1", "coded:raw", "coded:by_fill",
                    "refused:no_rig", "refused:clip_range", "refused:async_with_rebuild", "refused:warp_motion_stale",
                    "binding:rigid", "binding:skinned", "binding:morph", "binding:morph+skin",
                    "sample:before", "sample:after", "sample:key", "sample:between", "slerp:flip", "slerp:lerp", "slerp:slerp"]
                   + ["advance:%g" % a for a in af.ADVANCES] + ["lens:%d:%s" % (f, c) for f in (0, 1, 2) for c in ("camera", "no camera")]
                   + ["channel:%d:%s" % (p, i) for p in range(4) for i in ("step", "linear")])
LATE_SITUATIONS = (["pair:animated>%s" % k for k in KINDS] + ["pair:%s>animated" % k for k in KINDS]
                   + ["%s, a refused update_animated, set_rig and an accepted one" % k for k in ("set_skins", "set_morphs", "set_scene")]
                   + ["a request while a build is in flight", "adoption by a later update after WAIT", "adoption by rebuild_state(ADOPT)",
                      "an adopting update between two frames in flight", "an adoption inside a tracked interval",
                      "an update between snapshot and adoption", "a build ended by set_scene", "a build ended by REBUILD",
                      "warp_motion with a moved mesh", "warp_motion when nothing moved", "warp_motion after a step that did not know the motion",
                      "a stale G-buffer refused after an adoption, accepted after a fresh trace", "focus AUTO across a resize",
                      "a coded packet on the first frame of another size", "a coded packet on a frame of partial blocks",
                      "a coded packet on the (3, 50) frame"])


@pytest.fixture(scope="module")
def walked_late(oracle):
    out = {}
    for seed in af.LATE_DEFAULT_SEEDS:
        s = af.script(seed, late=True)
        model, _ = af.scene_of(s)
        out[seed] = (s, model, walk_late(s, model, oracle))
    return out


def test_a_late_script_is_a_pure_function_of_the_seed():
    for seed in (0, 2, 5):
        assert _same(af.script(seed, late=True), af.script(seed, late=True))
    orders = {tuple(o["op"] for o in af.script(seed, late=True)["ops"][5:]) for seed in range(8, 32) if seed % 8 not in (2, 5)}
    assert len(orders) >= 12, len(orders)


def test_every_late_script_does_something(walked_late, oracle):
    """Conditions, not measurements: ten operations, at most 2 refused calls, at least 3 frame groups with a chain, and every
    default script holds one of the new operations; the next 8 seeds, all drawn, keep the first three."""
    more = {}
    for seed in range(8, 16):
        s = af.script(seed, late=True)
        more[seed] = (s, None, walk_late(s, af.scene_of(s)[0], oracle))
    for seed, (s, _, (seen, refused, chained)) in list(walked_late.items()) + list(more.items()):
        assert len(s["ops"]) == af.OPS == 10
        assert refused <= 2 and chained >= 3, (seed, refused, chained)
        if seed in af.LATE_DEFAULT_SEEDS:
            assert any(x.startswith(NEW_OPS) for x in seen), seed


def test_the_late_default_seeds_reach_every_operation(walked_late):
    seen = set().union(*(w[2][0] for w in walked_late.values()))
    missing = [w for w in LATE_OPERATIONS if w not in seen]
    assert not missing, missing


def test_the_late_default_seeds_reach_every_situation(walked_late):
    seen = set().union(*(w[2][0] for w in walked_late.values()))
    missing = [w for w in LATE_SITUATIONS if w not in seen]
    assert not missing, missing


def test_late_shapes_and_budgets(walked_late):
    sizes = set()
    for seed, (s, model, _) in walked_late.items():
        c, (w, h) = s["config"], s["size"]
        sizes.add((w, h))
        assert max(c["spp"]) <= 4 and 1 <= c["max_depth"] <= 3 and len(s["rig"]["parent"]) <= 48
        assert (w, h) == af.BIG if c["chains_per_frame"] == 2 else (w, h) in af.SIZES
        if s["scene"][0] == "atrium":
            assert 500 <= s["scene"][1] <= 2000
    assert (3, 50) in sizes and {s["scene"][0] for s, _, _ in walked_late.values()} == {"cornell", "atrium"}


def test_late_dry_run_keeps_every_position_finite(walked_late, oracle):
    for seed, (s, model, _) in walked_late.items():
        vtx = am.dry_run(s, model, oracle)
        assert np.isfinite(vtx).all() and vtx.shape[0] == sum(m.vertex.shape[0] for m in model.meshes)


# what each late default seed's forced units (af.LATE_FORCED) are there for: the seed reaches it itself, so that a unit taken
# out of the table is missed even where another seed happens to draw the same thing
LATE_OWN = {
    0: ["adoption by a later update after WAIT", "focus AUTO across a resize", "a coded packet on the first frame of another size"],
    # ("an update between snapshot and adoption": what the script sets up; whether it happens is a race, see the docstring)
    1: ["set_skins, a refused update_animated, set_rig and an accepted one", "an update between snapshot and adoption", "lens:0:camera"],
    2: ["a request while a build is in flight", "an adopting update between two frames in flight", "lens:1:no camera"],
    3: ["set_morphs, a refused update_animated, set_rig and an accepted one", "warp", "coded:by_fill", "focus on its own trace"],
    4: ["set_scene, a refused update_animated, set_rig and an accepted one", "a build ended by set_scene", "a build ended by REBUILD",
        "warp_motion after a step that did not know the motion", "a coded packet on the (3, 50) frame"],
    5: ["refused:warp_motion_stale", "rebuild_state:0", "rebuild_state:2"],
    6: ["refused:async_with_rebuild", "focus_reset", "refused:clip_range", "lens:2:camera", "lens:0:no camera"],
    7: ["rebuild_state:3", "lens:1:camera"],
}


def test_each_late_default_seed_holds_its_own_units(walked_late):
    for seed, want in LATE_OWN.items():
        missing = [w for w in want if w not in walked_late[seed][2][0]]
        assert not missing, (seed, missing)


# sha256 over the late scripts of seeds 0 .. 31, computed with the generator as it was before the hdr family was added
LATE_SCRIPTS_DIGEST = "b9dd2b1fbe149d781aa76f68c4196fa1e1ace7183cc1e9b409e72f73c8b2d502"


def test_the_late_scripts_are_what_they_were():
    h = hashlib.sha256()
    for seed in range(32):
        _feed(h, af.script(seed, late=True))
    assert h.hexdigest() == LATE_SCRIPTS_DIGEST
    assert not any("hdr" in af.script(seed, late=True) or "variance" in o["chain"] for seed in (0, 9) for o in af.script(seed, late=True)["ops"] if o["op"] == "frame")


# ---- the hdr family ----------------------------------------------------------------------------------------------------------------
# what the library accepts (csrc/api_post.hip: variance_check, variance_filter_check, bloom_check; csrc/api_view.hip: quality_check)
def _variance_ok(c):
    return (1 <= c["history_cap"] <= 64 and 0 <= c["spatial_below"] <= c["history_cap"] + 1 and 1 <= c["spatial_radius"] <= 3
            and 0.0 <= c["depth_tolerance"] <= 1.0 and 0.0 <= c["normal_tolerance"] <= 4.0)


def walk_hdr(s):
    """walk() for an hdr script -> (set of names, refused operations, frames with a chain).  It follows on its own what decides
    which situation a chain is in: the tracking and the interval, the events since the last variance step, whether a moment
    history is alive, the size of the context's own variance image, the exposure state's last event and the background build
    ("no", "yes", or "maybe" once an update that may have adopted it has run)."""
    seen, refused, chained = set(), 0, 0
    ops, size = s["ops"], tuple(s["size"])
    # the head's mesh: the one all three updates of the first interval share
    head = set.intersection(*(set(o["poses"]) if o["kind"] != "animated" else {b["mesh"] for b in s["rig"]["bindings"]} for o in ops[1:4]))
    assert head
    rig = s["rig"]
    tracking = stepped = False
    moved = set()                                         # the meshes moved since the last temporal step
    events = set()                                        # what happened since the last variance step
    var_live, var_own, rendered = False, None, False
    ex_last, ex_any = None, False                         # the exposure state's last event; any step since the scene was set
    flight = "no"

    def update(u, where):
        nonlocal flight
        flag = u["rebuild"]
        meshes = {b["mesh"] for b in rig["bindings"]} if u["kind"] == "animated" else set(u["poses"])
        assert flag in (False, True, "async") and (u["kind"] != "animated" or rig is not None)
        if flag is True:
            flight = "no"
        elif meshes and flight == "yes":
            flight = "maybe"
        if flag == "async" and flight == "no":
            flight = "yes"
        moved.update(meshes)
        seen.add("update " + where)

    for i, op in enumerate(ops):
        kind = op["op"]
        if kind == "update":
            update(op, "alone")
        elif kind == "refused":
            refused += 1
            which = op["which"]
            seen.add("refused:" + which)
            if which == "vfilter_no_image":
                assert rendered and var_own != size and op["code"] == af.E_NO_FRAME
                assert ops[i - 1]["op"] == "frame" and ops[i - 2]["op"] == "resize" and ops[i - 1]["chain"]["variance"] is None
            elif which == "variance_bad_config":
                assert not _variance_ok(dict(af.HDR_VARIANCE_DEFAULTS, **{op["field"]: op["value"]})) and op["code"] == af.E_INVALID
                a, b = ops[i - 1], ops[i + 1] if i + 1 < len(ops) else None
                if a["op"] == "frame" and a["chain"]["variance"] is not None and b is not None and b["op"] == "frame" and b["chain"]["variance"] is not None:
                    seen.add("a refused config between two steps of one history")
            elif which == "bloom_bad_levels":
                assert not 1 <= op["value"] <= af.BLOOM_MAX_LEVELS and op["code"] == af.E_INVALID
            elif which == "quality_bad_ring":
                assert not 1 <= op["value"] <= 65536 and op["code"] == af.E_INVALID
        elif kind in ("set_skins", "set_morphs"):
            rig = None
        elif kind == "set_rig":
            rig = op["rig"]
        elif kind == "rebuild_state":
            if op["adopt"] and op["wait"] and flight == "yes":
                flight = "no"
            elif op["adopt"] and flight != "no":
                flight = "maybe"
        elif kind == "frame":
            n = len(op["views"])
            assert 1 <= n <= 3 and len(op["between"]) == n - 1
            for b in op["between"]:
                if b is not None and b["op"] == "update":
                    update(b, "between")
                elif b is not None:
                    refused += 1
            rendered = True
            c = op["chain"]
            v, f, bl, q = (c[k] for k in ("variance", "vfilter", "bloom", "quality"))
            ahead = set()
            if op["adopt_first"] and flight == "yes":
                ahead.add("an adoption")
                flight = "no"
            elif op["adopt_first"]:
                flight = "no" if flight == "no" else "maybe"
            if op["pre_chain"] is not None:
                u = op["pre_chain"]
                update(u, "between a render and its post chain")
                ahead.add({True: "a rebuild", "async": "a background build requested", False: "a refit"}[u["rebuild"]])
            chained += any(c[k] is not None for k in ("post", "expose", "focus", "last", "variance", "bloom", "quality")) or c["packet"]
            post = c["post"]
            assert post is None or post in po.VALID_STAGES
            has_t, has_m = post is not None and bool(post & po.TEMPORAL), post is not None and bool(post & po.MOTION)
            untracked_step = has_m and not stepped
            over_head = has_m and stepped and tracking and head <= moved
            if has_t:
                tracking = tracking or has_m
                stepped, moved = True, set()
            origin = src = "frame" if post is None else "post"
            if v is not None:
                seen.add("variance")
                assert _variance_ok(v["cfg"]) and v["motion"] == has_m and (v["gbuffer"] == "own" or has_t)
                assert v["cfg"]["history_cap"] in (2, 3, 16) and v["cfg"]["spatial_below"] in (0, 2, 4)
                seen.add("variance on " + ("the temporal G-buffer" if v["gbuffer"] == "temporal" else "its own trace"))
                seen.add("variance into " + ("the context's image" if v["own"] else "a caller's image"))
                if v["adopt"]:
                    assert flight == "yes" and v["gbuffer"] == "temporal"
                    seen.add("an adoption between the step and the variance call that takes its G-buffer")
                    flight = "no"
                if over_head:
                    seen.add("variance with motion over an interval that moved the head's mesh")
                if untracked_step:
                    seen.add("variance with motion from an untracked step")
                if post is None:
                    seen.add("variance with no post at all")
                elif not has_m:
                    seen.add("variance behind a post without MOTION")
                if size == (3, 50):
                    seen.add("variance on the (3, 50) frame")
                if size == af.BIG and s["config"]["chains_per_frame"] == 2:
                    seen.add("variance on the 192 x 128 two-chain frame")
                for e in events:
                    seen.add("variance after " + e)
                    # read at the pixel itself: a history that wrongly survived a reset that ends it would show, and so would one
                    # that wrongly ended at a reset that leaves it (which needs a history to be there)
                    if not has_m and (var_live or e in ENDS_THE_MOMENTS):
                        seen.add("variance without motion after " + e)
                events = set()
                for a in ahead:
                    seen.add("%s between the frames and a chain with a variance step" % a)
                    seen.add("an update or adoption ahead of a variance step on " + ("the temporal G-buffer" if v["gbuffer"] == "temporal" else "its own trace"))
                if var_live:
                    seen.add("a variance step that continues a history")
                var_live = True
                if v["own"]:
                    var_own = size
            if f is not None:
                assert v is not None and all(0 <= f["cfg"][k] <= 3 for k in af.ITS) and f["cfg"]["demodulate"] in (0, 1)
                assert all(1e-3 < f["cfg"][k] < 1e3 for k in ("luminance_sigma", "normal_sigma", "depth_sigma"))
                assert (f["input"] == "accum" or post is not None) and (f["variance"] == "given" or v["own"])
                seen.add("vfilter")
                seen.add("a filter on " + ("the context's variance image" if f["variance"] == "own" else "a caller's variance image" if not v["own"] else "the context's image by its address"))
                seen.add("a filter of " + ("the post colour" if f["input"] == "post" else "the accum buffer"))
                seen.add("a filter into " + ("the context's buffers" if f["out_own"] else "a caller's buffers"))
                if not any(f["cfg"][k] for k in af.ITS):
                    seen.add("a filter with no iterations")
                origin = src = "vfilter"
            if c["focus"] is not None:
                origin = src = "focus"
            if bl is not None:
                d = bl["cfg"]
                assert 0 <= d["flags"] <= 7 and 1 <= d["levels"] <= af.BLOOM_MAX_LEVELS and all(0.0 <= d[g] <= 1.0 for g in af.GAIN_NAMES)
                assert 1e-3 < d["threshold"] < 1e3 and 1e-3 < d["exposure"] < 1e3 and 0 <= d["knee"] < 1e3 and 0 <= d["intensity"] <= 1 and 0 <= d["spread"] <= 1
                assert not bl["in_place"] or src in ("vfilter", "focus")
                seen.add("bloom")
                seen.add("bloom flags %d" % d["flags"])
                seen.add("bloom levels %d" % d["levels"])
                if bl["in_place"]:
                    seen.add("bloom in place")
                if d["flags"] & af.STATE:
                    seen.add("bloom state " + {None: "before any expose step", "reset": "after expose_reset", "auto": "after an AUTO step", "fixed": "after a FIXED step"}[ex_last])
                origin = "bloom"
            if c["expose"] is not None:
                ex_last = "auto" if c["expose"]["mode"] == af.AUTO else "fixed"
                ex_any = True
                origin = "expose"
            if q is not None:
                assert q["flags"] in (0, 1, 2, 3) and q["ring_width"] in (1, 3, 16) and q["ref"] != origin and (q["ref"] == "frame" or post is not None)
                seen.add("quality")
                seen.add("quality flags %d" % q["flags"])
                seen.add("quality into " + ("the context's record" if q["record_own"] else "a caller's record"))
                seen.add("quality against " + ("the post step's rgba8" if q["ref"] == "post" else "the frame buffer"))
                if q["classes"]:
                    seen.add("quality with a class map")
            if v is not None and f is not None and bl is not None and q is not None:
                if n == 3 and s["config"]["frames_in_flight"] == 2:
                    seen.add("three views in flight ahead of all four stages")
            if op["moved_on"] is not None and f is not None and bl is not None and bl["cfg"]["flags"] & af.GAINS and q is not None and q["classes"]:
                seen.add("moved_on ahead of the variance filter, bloom with GAINS and quality with a class map")
            la = c["last"]
            if la is not None and la["stage"] == "warp_motion":
                assert has_t and has_m
        elif kind == "resize":
            events.add("a resize to the same size" if tuple(op["size"]) == size else "a resize to another size")
            size = tuple(op["size"])
            stepped, var_live, var_own, rendered = False, False, None, False
        elif kind == "set_scene":
            events.add("set_scene")
            rig, flight = None, "no"
            tracking = stepped = var_live = False
            moved = set()
            ex_last, ex_any = None, False
        elif kind == "temporal_reset":
            events.add("temporal_reset")
            stepped = False
        elif kind == "expose_reset":
            events.add("expose_reset")
            ex_last = "reset" if ex_any else None
        elif kind == "variance_reset":
            seen.add("variance_reset")
            events.add("variance_reset")
            var_live = False
        else:
            assert kind == "focus_reset", kind
            events.add("focus_reset")
    return seen, refused, chained


ENDS_THE_MOMENTS = ("variance_reset", "a resize to the same size", "a resize to another size", "set_scene")
LEAVES_THE_MOMENTS = ("temporal_reset", "expose_reset", "focus_reset")
HDR_OPERATIONS = ["variance", "vfilter", "bloom", "quality", "variance_reset", "refused:vfilter_no_image", "refused:variance_bad_config",
                  "refused:bloom_bad_levels", "refused:quality_bad_ring", "variance on the temporal G-buffer", "variance on its own trace",
                  "variance into the context's image", "variance into a caller's image", "a filter of the post colour", "a filter of the accum buffer",
                  "a filter into the context's buffers", "a filter into a caller's buffers", "quality against the post step's rgba8",
                  "quality against the frame buffer"]
HDR_SITUATIONS = (["variance with motion over an interval that moved the head's mesh", "variance with motion from an untracked step",
                   "variance behind a post without MOTION", "variance with no post at all", "variance on the (3, 50) frame",
                   "variance on the 192 x 128 two-chain frame"]
                  + ["variance after " + e for e in ("variance_reset", "temporal_reset", "expose_reset", "a resize to the same size", "a resize to another size", "set_scene")]
                  + ["variance without motion after a resize to the same size", "variance without motion after set_scene"]
                  + ["variance without motion after " + e for e in LEAVES_THE_MOMENTS]      # (on a live history: it must go on)
                  + ["%s between the frames and a chain with a variance step" % a for a in ("a rebuild", "a background build requested", "an adoption")]
                  + ["an update or adoption ahead of a variance step on its own trace", "an update or adoption ahead of a variance step on the temporal G-buffer",
                     "an adoption between the step and the variance call that takes its G-buffer",
                     "moved_on ahead of the variance filter, bloom with GAINS and quality with a class map", "three views in flight ahead of all four stages",
                     "bloom state before any expose step", "bloom state after expose_reset", "bloom state after an AUTO step", "bloom state after a FIXED step",
                     "bloom in place", "bloom levels 1", "bloom levels %d" % af.BLOOM_MAX_LEVELS, "a filter with no iterations",
                     "a filter on the context's variance image", "a filter on a caller's variance image", "quality into the context's record",
                     "quality into a caller's record", "quality with a class map", "a refused config between two steps of one history",
                     "a variance step that continues a history"]
                  + ["quality flags %d" % k for k in range(4)]
                  + ["refused:" + k for k in ("vfilter_no_image", "variance_bad_config", "bloom_bad_levels", "quality_bad_ring")])


@pytest.fixture(scope="module")
def walked_hdr():
    out = {}
    for seed in af.HDR_DEFAULT_SEEDS:
        s = af.script(seed, hdr=True)
        model, _ = af.scene_of(s)
        out[seed] = (s, model, walk_hdr(s))
    return out


def test_an_hdr_script_is_a_pure_function_of_the_seed():
    for seed in (0, 2, 5):
        assert _same(af.script(seed, hdr=True), af.script(seed, hdr=True))
    for seed in (0, 3, 9):                               # the late script's scene, size, config, skins, morphs and rig; operations of its own
        a, b = af.script(seed, hdr=True), af.script(seed, late=True)
        assert all(_same(a[k], b[k]) for k in ("scene", "size", "config", "post", "skins", "morphs", "rig")) and not _same(a["ops"], b["ops"])
    orders = {tuple(o["op"] for o in af.script(seed, hdr=True)["ops"][5:]) for seed in range(8, 32) if seed % 8 not in (2, 5)}
    assert len(orders) >= 12, len(orders)


def test_every_hdr_script_does_something(walked_hdr):
    """Ten operations, at most 2 refused calls, a frame group in the tail, and every chain entry valid (walk_hdr asserts the
    library's ranges): for the default seeds and the next 24, all drawn; every default script holds one of the new stages."""
    more = {}
    for seed in range(8, 32):
        s = af.script(seed, hdr=True)
        more[seed] = (s, None, walk_hdr(s))
    for seed, (s, _, (seen, refused, chained)) in list(walked_hdr.items()) + list(more.items()):
        assert len(s["ops"]) == af.OPS == 10
        assert refused <= af.MAX_REFUSED and chained >= 3 and any(o["op"] == "frame" for o in s["ops"][5:]), (seed, refused, chained)
        assert "variance" in seen, seed
    drawn = set().union(*(w[2][0] for w in more.values()))
    assert len({x for x in drawn if x.startswith("bloom flags")}) == 8       # every subset of KARIS, GAINS and EXPOSURE_STATE is drawn


def test_the_hdr_default_seeds_reach_every_operation(walked_hdr):
    seen = set().union(*(w[2][0] for w in walked_hdr.values()))
    missing = [w for w in HDR_OPERATIONS if w not in seen]
    assert not missing, missing


def test_the_hdr_default_seeds_reach_every_situation(walked_hdr):
    """A variance step with motion from an interval in which the head's mesh moved, from an untracked step (w = 0 everywhere), with
    no motion (a post without MOTION, no post at all); on the (3, 50) frame and on the 192 x 128 two-chain frame; after each of
    variance_reset, temporal_reset, expose_reset, a resize to the same size, to another size and set_scene, and with no motion (so
    that the history is read at the pixel itself and a reset's effect on it shows) after a resize to the same size and set_scene,
    which end the moments, and on a live history after temporal_reset, expose_reset and focus_reset, which leave them; an update with a
    rebuild, one that requests a background build and an adoption, each between the frames and a chain with a variance step, on
    its own trace and on the temporal G-buffer; moved_on ahead of the filter, bloom with GAINS and quality with a class map; three
    views with two frames in flight ahead of all four stages; bloom with EXPOSURE_STATE before any expose step, after
    expose_reset, after an AUTO and after a FIXED step; bloom in place, with 1 level and with 8; a filter with no iterations, one
    on the context's image (variance = NULL) and one on a caller's; quality into the context's record and a caller's, with each
    flag subset; each of the four refusals."""
    seen = set().union(*(w[2][0] for w in walked_hdr.values()))
    missing = [w for w in HDR_SITUATIONS if w not in seen]
    assert not missing, missing


def test_hdr_shapes_and_budgets(walked_hdr):
    sizes = set()
    for seed, (s, model, _) in walked_hdr.items():
        c, (w, h) = s["config"], s["size"]
        sizes.add((w, h))
        assert max(c["spp"]) <= 4 and 1 <= c["max_depth"] <= 3
        assert (w, h) == af.BIG if c["chains_per_frame"] == 2 else (w, h) in af.SIZES
        assert all(tuple(o["size"]) in af.SIZES + [af.BIG] for o in s["ops"] if o["op"] == "resize")
    assert (3, 50) in sizes and af.BIG in sizes and {s["scene"][0] for s, _, _ in walked_hdr.values()} == {"cornell", "atrium"}


def test_hdr_dry_run_keeps_every_position_finite(walked_hdr, oracle):
    for seed, (s, model, _) in walked_hdr.items():
        vtx = am.dry_run(s, model, oracle)
        assert np.isfinite(vtx).all() and vtx.shape[0] == sum(m.vertex.shape[0] for m in model.meshes)


# what each hdr default seed's forced units and head chains (af.HDR_FORCED, af.HDR_HEAD_CHAIN) are there for
HDR_OWN = {
    0: ["variance after variance_reset", "a refused config between two steps of one history", "a filter with no iterations",
        "a filter on the context's variance image", "an adoption between the step and the variance call that takes its G-buffer", "quality into a caller's record"],
    1: ["three views in flight ahead of all four stages", "variance after temporal_reset", "variance without motion after temporal_reset",
        "variance with motion from an untracked step", "refused:bloom_bad_levels", "bloom state after a FIXED step"],
    2: ["variance after expose_reset", "bloom state after expose_reset", "a rebuild between the frames and a chain with a variance step", "refused:quality_bad_ring"],
    3: ["variance after a resize to the same size", "variance without motion after a resize to the same size", "a background build requested between the frames and a chain with a variance step",
        "an update or adoption ahead of a variance step on the temporal G-buffer", "variance on the 192 x 128 two-chain frame"],
    4: ["variance on the (3, 50) frame", "variance after a resize to another size", "refused:vfilter_no_image", "bloom in place", "bloom levels 1",
        "bloom levels %d" % af.BLOOM_MAX_LEVELS],
    5: ["variance after set_scene", "variance without motion after set_scene", "an adoption between the frames and a chain with a variance step", "bloom state before any expose step"],
    6: ["variance with no post at all", "variance behind a post without MOTION", "a filter on a caller's variance image", "quality flags 2", "quality flags 3",
        "variance without motion after focus_reset"],
    7: ["moved_on ahead of the variance filter, bloom with GAINS and quality with a class map", "quality into the context's record", "quality with a class map",
        "variance without motion after expose_reset"],
}


def test_each_hdr_default_seed_holds_its_own_units(walked_hdr):
    for seed, want in HDR_OWN.items():
        missing = [w for w in want if w not in walked_hdr[seed][2][0]]
        assert not missing, (seed, missing)


# sha256 over the hdr scripts of seeds 0 .. 31
HDR_SCRIPTS_DIGEST = "c98b0d9b11011f4e389da841ae8831b29acd7abc817c10a1484f869c349b53a5"


def test_the_hdr_scripts_are_what_they_were():
    h = hashlib.sha256()
    for seed in range(32):
        _feed(h, af.script(seed, hdr=True))
    assert h.hexdigest() == HDR_SCRIPTS_DIGEST


def test_the_restatements_of_an_hdr_chain_stay_finite_and_quick():
    """No renderer: for every frame size and every chain config of the default hdr scripts, variance_ref.moments twice (the second
    on the first's history, with motion), vfilter, bloom_ref.bloom and quality_ref.quality on a synthetic frame -- a tilted plane
    with a hole of misses, a noisy colour with black pixels and spikes.  Finite inputs give finite outputs, and the slowest size's
    time is printed and bounded: the model runs these after every chain."""
    import time
    import bloom_ref as br
    import quality_ref as qr
    import variance_ref as vr
    cam = dict(eye=(0.0, 0.0, 0.0), U=(1.0, 0.0, 0.0), V=(0.0, 1.0, 0.0), W=(0.0, 0.0, -1.0))
    slowest = {}
    for seed in af.HDR_DEFAULT_SEEDS:
        s = af.script(seed, hdr=True)
        size, c = tuple(s["size"]), s["config"]
        for op in s["ops"]:
            if op["op"] == "resize":
                size = tuple(op["size"])
            ch = op["chain"] if op["op"] == "frame" else None
            if ch is None or ch["variance"] is None:
                continue
            w, h = size
            rng = np.random.default_rng(seed)
            Y, X = np.mgrid[0:h, 0:w].astype(F)
            z = (F(5.0) + F(0.05) * X + F(0.02) * Y).astype(F)
            pos = np.stack([(X - w / 2) * z / w, (Y - h / 2) * z / w, -z, z], axis=-1).astype(F)
            pos[h // 3:h // 2, w // 3:w // 2, 3] = -1.0
            nrm = np.zeros((h, w, 4), F)
            nrm[..., 2] = 1.0
            gb = dict(position=pos, normal=nrm, albedo=rng.uniform(0, 1, (h, w, 4)).astype(F))
            color = np.exp2(rng.uniform(-8, 2, (h, w, 4))).astype(F)
            color[rng.random((h, w)) < 0.1, :3] = 0.0
            color[rng.random((h, w)) < 0.02, :3] = 500.0
            gaze = op["views"][-1]["gaze"]
            fill, pas = vr.fills(w, h, gaze, c["r_inner"], c["r_outer"], c["uniform"])
            t0 = time.perf_counter()
            vc = dict(vr.MOMENT_DEFAULTS, **ch["variance"]["cfg"])
            hist, var = vr.moments(None, color, gb, cam, fill, None, vc)
            mv = np.zeros((h, w, 4), F)
            mv[..., :2], mv[..., 2], mv[..., 3] = rng.uniform(-1.5, 1.5, (h, w, 2)), hist[..., 3], 1.0
            hist, var = vr.moments(hist, color, gb, cam, fill, mv, vc)
            assert np.isfinite(hist).all() and np.isfinite(var).all() and (hist[..., 2] >= 1).all()
            out = color
            if ch["vfilter"] is not None:
                fc = dict(vr.FILTER_DEFAULTS, **ch["vfilter"]["cfg"])
                out, _ = vr.vfilter(color, var, gb, fill, vr.iteration_map(fill, pas, fc, c["uniform"]), fc)
                assert np.isfinite(out).all()
            if ch["bloom"] is not None:
                import reconstruct_ref as rr
                got = br.bloom(None, out, ch["bloom"]["cfg"], None, rr.writers(w, h, gaze, c["r_inner"], c["r_outer"], c["uniform"])[0], c["uniform"])
                assert np.isfinite(got["color"]).all() and np.isfinite(got["pyramid"]).all()
                out = got["color"]
            if ch["quality"] is not None:
                code = lambda img: np.clip(np.asarray(img)[..., 0] * 255.0, 0, 255).astype(np.uint32) * np.uint32(0x010101)
                q = qr.quality(code(out), code(color), qr.classes_of_frame(w, h, gaze, c["r_inner"], c["r_outer"], c["uniform"]), gaze,
                               dict(flags=ch["quality"]["flags"], ring_width=ch["quality"]["ring_width"]))
                assert sum(q["pixels"]) == w * h
            slowest[size] = max(slowest.get(size, 0.0), time.perf_counter() - t0)
    print("the restatements of one hdr chain, slowest per size:", {k: round(v, 3) for k, v in sorted(slowest.items())})
    assert af.BIG in slowest and (3, 50) in slowest
    assert slowest[af.BIG] < 5.0                          # (a few seconds at 192 x 128 would ask for fewer periphery iterations)
