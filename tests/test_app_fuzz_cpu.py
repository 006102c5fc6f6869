"""tests/app_fuzz.py without a GPU: the scripts are a pure function of the seed, the default seeds reach every operation and every
situation the sweep of tests/test_app_fuzz_gpu.py is there for, every pose drawn as valid passes the overflow rule of its kind
and every pose drawn as refused does not, and a dry run of the positions (tests/app_model.dry_run) stays finite."""
import numpy as np
import pytest

import app_fuzz as af
import app_model as am
import morph_ref as mr
import post_ref as po
import skin_ref as sk
import transform_ref as tf

KINDS = af.KINDS


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
