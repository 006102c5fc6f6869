"""The rules and layouts of the animation set-up (csrc/fovpt_animplan.h: plan_skins, plan_morphs, plan_rig and the overflow rules of
the fovpt_update_* calls) without a GPU.  The header is compiled into the stand-alone program of tests/cpp/anim_plan_test.cpp
under the address and undefined-behaviour sanitizers (nothing preloaded).  The program is given every array at its real length,
apart from the count the description states, so that a read beyond what the earlier rules admitted is the sanitizer's to report.

The shared rejection cases of tests/anim_cases.py are refused with the code and the text of tests/golden/anim_rejections.json (the
library's before the rules moved here); the header's verdict is the restatements' (rig_ref.accepted, morph_ref.accepted,
skin_ref.accepted, transform_ref.accepted); and an accepted plan is checked against the description it was made from."""
import os
import subprocess

import numpy as np
import pytest

import anim_cases as ac
import morph_ref as mr
import rig_ref as rg
import skin_ref as sk
import transform_ref as tf
from fovpathtracing_optixcodelatest_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fovpathtracing_optixcodelatest_amd", "csrc")
F = np.float32
E_INVALID = -1
DOUBLE_TABLES = ("S", "B", "D")
# What a list's opening checks refuse (Listed::open of csrc/api_animate.hip: the count, the array, the flags), which need a context
OPENING = ("num below 0",)
# What anim_list_mesh refuses in the lists of the update calls
LISTING = ("mesh above", "mesh below", "listed twice")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("anim_plan") / "anim_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "anim_plan_test.cpp"), "-o", exe])

    def run(commands):
        """One answer per command: dict(code, text, and the tables of an accepted plan as integer arrays)."""
        res = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        assert "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-4000:]
        out, cur = [], {}
        for line in res.stdout.splitlines():
            if line == "end":
                out.append(cur)
                cur = {}
            elif line.startswith("text "):
                cur["text"] = line[5:]
            else:
                f = line.split()
                if f[0] == "code":
                    cur["code"] = int(f[1])
                    continue
                doubles = f[0].rstrip("0123456789") in DOUBLE_TABLES     # (as their bits)
                v = np.array([int(x) for x in f[2:]], np.uint64 if doubles else np.int64)
                assert len(v) == int(f[1])
                cur[f[0]] = v.view(np.float64) if doubles else v
        assert len(out) == len(commands), (len(out), len(commands))
        return out
    return run


def as_floats(v):
    return np.asarray(v, np.int64).astype(np.uint32).view(F)


# ---- serialising a description -----------------------------------------------------------------------------------------------------
def vals(a, dtype):
    """The values, floats and doubles as their bits."""
    a = np.ascontiguousarray(a, dtype).reshape(-1)
    if dtype is F:
        a = a.view(np.uint32)
    elif dtype is np.float64:
        a = a.view(np.uint64)
    return " ".join(str(int(x)) for x in a)


def arr(a, dtype):
    """An array as the driver reads it: its real length and its values; -1 for None."""
    return "-1" if a is None else ("%d %s" % (np.asarray(a).size, vals(a, dtype))).strip()


def f64(x):
    return str(int(np.array([x], np.float64).view(np.uint64)[0]))


def scene(nv, skins=None, morphs=None):
    """The scene view as csrc/api_animate.hip builds it: skins {mesh: joint count}, morphs {mesh: (targets, entries)}; a skinned
    mesh's first joint and a morphed mesh's first weight are the running sums in mesh order."""
    skins, morphs = skins or {}, morphs or {}
    out, pal_first, w_first = [], 0, 0
    for m, n in enumerate(nv):
        nj, (nt, ne) = skins.get(m, 0), morphs.get(m, (0, 0))
        out.append((n, nj, pal_first, nt, w_first, ne))
        pal_first, w_first = pal_first + nj, w_first + nt
    return out


def scene_text(sc):
    return " ".join([str(len(sc))] + ["%d %d %d %d %d %d" % m for m in sc])


def skins_text(sc, entries, num=None):
    t = ["skins", scene_text(sc), str(len(entries) if num is None else num), str(len(entries))]
    for e in entries:
        t += ["%d %d %d %d" % (e["mesh"], e["nv"], e["nj"], e["reserved"]), arr(e["joints"], np.uint16), arr(e["weights"], F)]
    return " ".join(t)


def morphs_text(sc, entries, num=None, command="morphs"):
    t = [command, scene_text(sc), str(len(entries) if num is None else num), str(len(entries))]
    for e in entries:
        t += ["%d %d %d %d" % (e["mesh"], e["nv"], e["nt"], e["reserved"]), str(-1 if e["targets"] is None else len(e["targets"]))]
        for T in e["targets"] or ():
            t += ["%d %d" % (T["count"], T["reserved"]), arr(T["index"], np.uint32), arr(T["delta"], F)]
    return " ".join(t)


def rig_text(sc, d):
    t = ["rig", scene_text(sc), "%d %d %d %d %d %d" % (d["reserved0"], d["reserved1"], d["reserved2"], d["num_nodes"], d["num_bindings"], d["num_clips"])]
    t.append(str(-1 if d["nodes"] is None else len(d["nodes"])))
    for N in d["nodes"] or ():
        t += [str(N["parent"]), vals(np.concatenate([N["translation"], N["rotation"], N["scale"]]), F)]
    t.append(str(-1 if d["bindings"] is None else len(d["bindings"])))
    for B in d["bindings"] or ():
        t += ["%d %d %d %d" % (B["mesh"], B["node"], B["num_joints"], B["reserved"]), arr(B["joint_nodes"], np.uint16), arr(B["inverse_bind"], F)]
    t.append(str(-1 if d["clips"] is None else len(d["clips"])))
    for K in d["clips"] or ():
        t += ["%d %d" % (K["num_channels"], K["reserved"]), str(-1 if K["channels"] is None else len(K["channels"]))]
        for H in K["channels"] or ():
            t += ["%d %d %d %d" % (H["target"], H["path"], H["interpolation"], H["num_keys"]), arr(H["times"], F), arr(H["values"], F)]
    return " ".join(t)


def transform_text(mesh, m, A):
    return "transform %d %s %s" % (mesh, f64(A), vals(m, F))


def palette_text(who, mesh, nj, m, S, B):
    return "palette %s %d %d %s %s %s" % (who, mesh, nj, f64(S), f64(B), arr(m, F))


def weights_text(mesh, nt, w, D, A):
    return "weights %d %d %s %s %s" % (mesh, nt, arr(w, F), arr(D, np.float64), f64(A))


def absmax(vertex):
    v = np.asarray(vertex, F)
    return float(np.abs(v.astype(np.float64)).max()) if v.size else 0.0


def first_refusal(answers):
    return next((a for a in answers if a["code"]), answers[-1])


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    return scenes.cornell_box()


def nv_of(model):
    return [m.vertex.shape[0] for m in model.meshes]


def entries_of(targets, n):
    return sum(len(mr.split(t, n)[0]) for t in targets)


@pytest.fixture(scope="module")
def rig_fixture(base):
    """(scene view, skins, morphs, rig, description) of test_rig_gpu's rejection test."""
    skins, morphs, rig = ac.rig_scene(base)
    nv = nv_of(base)
    sc = scene(nv, {k: s[2] for k, s in skins.items()}, {k: (len(t), entries_of(t, nv[k])) for k, t in morphs.items()})
    return sc, {k: s[2] for k, s in skins.items()}, {k: len(t) for k, t in morphs.items()}, rig, ac.describe_rig(rig)


# ---- 1. plain C++ ------------------------------------------------------------------------------------------------------------------
def test_the_header_is_plain_cpp_and_defines_the_pods_once(driver):
    """Standard headers and include/fovpt.h only, no HIP, so that g++ compiles it alone (the driver's build); the three PODs both
    sides need have one definition each, here, and the device header includes it."""
    text = open(os.path.join(CSRC, "fovpt_animplan.h")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes and all(i.startswith("<") for i in includes[:-1]) and includes[-1] == '"../../include/fovpt.h"'
    assert not any(i.startswith("<hip") for i in includes)
    assert not any(word in text for word in ("hipStream", "hipEvent", "hipError", "hipMalloc", "__global__", "__device__", "__host__", "fovpt_ctx*", "fovpt_ctx::"))
    sources = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".h", ".hip", ".cpp"))}
    for name in ("RigChannel", "RigWeights", "MorphEntry", "RigBound"):
        where = [f for f, s in sources.items() if "struct %s {" % name in s]
        assert where == ["fovpt_animplan.h"], (name, where)
    assert '#include "fovpt_animplan.h"' in sources["fovpt_device.h"]
    # no rule and no layout is left beside the header: the entry points hand the plans' texts on
    api = sources["api_animate.hip"]
    for word in ("rig_norm_ok(", "rig_place(", "0x1p127", "mesh %d is listed twice", "could overflow", "squared norm", "strictly ascending", "isfinite(T.", "isfinite(H."):
        assert word not in api, word
    alone = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", CSRC, "-x", "c++", "-"], input='#include "fovpt_animplan.h"\n',
                           capture_output=True, text=True)
    assert alone.returncode == 0, alone.stderr[-2000:]


# ---- 2. the shared cases are refused, with the recorded text ---------------------------------------------------------------------------
def test_every_shared_rig_case_is_refused_with_the_recorded_text(driver, rig_fixture):
    sc, _, _, rig, plain = rig_fixture
    cases = ac.rig_cases(rig)
    answers = driver([rig_text(sc, plain)] + [rig_text(sc, ac.changed(plain, changes)) for _, changes in cases])
    assert answers[0]["code"] == 0, answers[0]
    for (name, _), a in zip(cases, answers[1:]):
        assert a["code"] == E_INVALID and "parent" not in a, name
        ac.assert_recorded("rig", name, a["code"], a["text"])


def test_every_shared_skin_case_is_refused_with_the_recorded_text(driver, base):
    skins = ac.skin_scene(base)
    sc = scene(nv_of(base), {k: s[2] for k, s in skins.items()})
    cases = [c for c in ac.skin_set_cases(base, skins) if c[0] not in OPENING]
    assert len(cases) == len(ac.skin_set_cases(base, skins)) - 1
    for (name, _, _), a in zip(cases, driver([skins_text(sc, entries, n) for _, entries, n in cases])):
        assert a["code"] == E_INVALID and "S" not in a, name
        ac.assert_recorded("skins", name, a["code"], a["text"])


def test_every_shared_morph_case_is_refused_with_the_recorded_text(driver, base):
    morphs, skins = ac.morph_scene(base)
    nv = nv_of(base)
    sc = scene(nv, {k: s[2] for k, s in skins.items()}, {k: (len(t), entries_of(t, nv[k])) for k, t in morphs.items()})
    cases = [c for c in ac.morph_set_cases(base) if c[0] not in OPENING]
    assert len(cases) == len(ac.morph_set_cases(base)) - 1
    for (name, _, _), a in zip(cases, driver([morphs_text(sc, entries, n) for _, entries, n in cases])):
        assert a["code"] == E_INVALID and "off_first" not in a, name
        ac.assert_recorded("morphs", name, a["code"], a["text"])


def _listing(who, nmesh, meshes):
    return "list %s %d %d %s" % (who, nmesh, len(meshes), " ".join(str(m) for m in meshes))


def test_every_shared_transform_case_is_refused_with_the_recorded_text(driver, base):
    who, n_header = "fovpt_update_transforms", 0
    for name, entries, n, flags, rule in ac.transform_cases(base):
        if name in LISTING:
            a = driver([_listing(who, len(base.meshes), [m for m, _ in entries])])[0]
        elif rule:
            a = first_refusal(driver([transform_text(mesh, m, absmax(base.meshes[mesh].vertex)) for mesh, m in entries]))
        else:
            continue                                                      # the opening checks: the count and the flags
        n_header += 1
        ac.assert_recorded("transforms", name, a["code"], a["text"])
    assert n_header == 9


def test_the_overflow_cases_of_update_skinned_are_refused_with_the_recorded_text(driver, base):
    who, skins, n_header = "fovpt_update_skinned", ac.skin_scene(base), 0
    for name, entries, n, flags, rule in ac.skin_pose_cases(base, ac.cornell_poses(base)):
        if name in LISTING:
            a = driver([_listing(who, len(base.meshes), [e["mesh"] for e in entries])])[0]
        elif rule:
            a = first_refusal(driver([palette_text(who, e["mesh"], e["nj"], e["m"], sk.weight_sum(skins[e["mesh"]][1]), absmax(base.meshes[e["mesh"]].vertex))
                                      for e in entries]))
        else:
            continue                                                      # the opening checks and what is checked against the context's skins
        n_header += 1
        ac.assert_recorded("skinned", name, a["code"], a["text"])
    assert n_header == 11


def test_the_overflow_cases_of_update_morphed_are_refused_with_the_recorded_text(driver, base):
    who, (morphs, skins), n_header = "fovpt_update_morphed", ac.morph_scene(base), 0
    nv = nv_of(base)
    for name, entries, n, flags, rule in ac.morph_pose_cases(base, morphs, ac.cornell_weights()):
        if name in LISTING:
            a = driver([_listing(who, len(base.meshes), [e["mesh"] for e in entries])])[0]
        elif rule:
            a = dict(code=0)
            for e in entries:                                             # as the entry point goes: a pose's weights, then its palette with their B
                m = e["mesh"]
                a = driver([weights_text(m, e["nt"], e["weights"], mr.target_max(morphs[m], nv[m]), absmax(base.meshes[m].vertex))])[0]
                if not a["code"] and e["nj"]:
                    assert a["B"][0] == mr.bound(base.meshes[m].vertex, morphs[m], e["weights"])
                    a = driver([palette_text(who, m, e["nj"], e["m"], sk.weight_sum(skins[m][1]), a["B"][0])])[0]
                if a["code"]:
                    break
        else:
            continue
        n_header += 1
        ac.assert_recorded("morphed", name, a["code"], a["text"])
    assert n_header == 15


# ---- 3. the restatements agree on acceptance ---------------------------------------------------------------------------------------
def test_rig_ref_accepts_the_fixture_and_refuses_each_case_it_can_state(rig_fixture):
    """The restatement alone, before it is relied on."""
    sc, skins, morphs, rig, plain = rig_fixture
    assert rg.accepted(rig, len(sc), skins, morphs) and rg.accepted(ac.rig_of(plain), len(sc), skins, morphs)
    stated = [(name, changes) for name, changes in ac.rig_cases(rig) if name not in ac.RIG_CASES_BEYOND_THE_RESTATEMENT]
    assert len(stated) == len(ac.rig_cases(rig)) - len(ac.RIG_CASES_BEYOND_THE_RESTATEMENT) == 43
    for name, changes in stated:
        assert not rg.accepted(ac.rig_of(ac.changed(plain, changes)), len(sc), skins, morphs), name


def _seeded_rig(seed):
    """A random rig over a scene of 9 meshes: skinned, skinned and morphed, morphed and rigid bindings in a random order, and,
    for two seeds in three, one change that may or may not break a rule."""
    rng = np.random.default_rng(5000 + seed)
    n = int(rng.integers(1, 40))
    rig = rg.random_rig(rng, n, max_depth=(None, 3, 12)[seed % 3], scales=bool(seed % 2), chains=0.5 * (seed % 2))
    nv = [int(x) for x in rng.integers(3, 30, 9)]
    skins, morphs, bindings = {}, {}, []
    for k in range(len(nv)):
        kind = rng.choice(["skin", "both", "morph", "rigid", "none"])
        if kind in ("skin", "both"):
            skins[k] = int(rng.integers(1, 9))
            nodes = rng.integers(0, n, skins[k]).astype(np.uint16)
            bindings.append(dict(mesh=k, joint_nodes=nodes, inverse_bind=rg.inverse_bind_of(rig, nodes)))
        if kind in ("both", "morph"):
            morphs[k] = int(rng.integers(1, 5))
            if kind == "morph":
                bindings.append(dict(mesh=k))
            keys = int(rng.integers(1, 4))
            rig["clips"][0].append(rg.channel(k, rg.WEIGHTS, np.cumsum(rng.uniform(0.2, 1.0, keys)), rng.uniform(-1, 2, (keys, morphs[k]))))
        if kind == "rigid":
            bindings.append(dict(mesh=k, node=int(rng.integers(0, n))))
    rig["bindings"] = [bindings[i] for i in rng.permutation(len(bindings))]
    d = ac.describe_rig(rig)
    change = seed % 3
    if change == 1:                                                       # a rotation's norm on either side of the rule
        d["nodes"][int(rng.integers(0, n))]["rotation"] *= F(rng.choice([0.49, 0.51, 1.99, 2.01]))
    if change == 2 and d["clips"][0]["channels"]:                         # a channel aimed somewhere else: out of range, twice, or fine
        H = d["clips"][0]["channels"][int(rng.integers(0, len(d["clips"][0]["channels"])))]
        H["target"] = int(rng.integers(-1, max(n, len(nv)) + 1))
    sc = scene(nv, skins, {k: (t, 3 * t) for k, t in morphs.items()})
    return sc, skins, morphs, d


def test_the_verdict_on_rigs_is_rig_refs(driver, rig_fixture):
    sc, skins, morphs, rig, plain = rig_fixture
    stated = [(name, changes) for name, changes in ac.rig_cases(rig) if name not in ac.RIG_CASES_BEYOND_THE_RESTATEMENT]
    for (name, changes), a in zip(stated, driver([rig_text(sc, ac.changed(plain, changes)) for _, changes in stated])):
        assert (a["code"] == 0) == rg.accepted(ac.rig_of(ac.changed(plain, changes)), len(sc), skins, morphs), name
    seeded = [_seeded_rig(seed) for seed in range(36)]
    want = [rg.accepted(ac.rig_of(d), len(s), sk_, mo) for s, sk_, mo, d in seeded]
    assert all(want[0::3]) and 0 < sum(want[1::3]) < 12 and 0 < sum(want[2::3]) < 12, want      # the seed set has both answers
    got = [a["code"] == 0 for a in driver([rig_text(s, d) for s, _, _, d in seeded])]
    assert got == want


def _skin_entry(mesh, nv, skin):
    return dict(mesh=mesh, nv=nv, nj=skin[2], reserved=0, joints=np.ascontiguousarray(skin[0], np.uint16), weights=np.ascontiguousarray(skin[1], F))


def _target_entry(t, n):
    if isinstance(t, tuple):
        return dict(count=len(t[0]), reserved=0, index=np.ascontiguousarray(t[0], np.uint32), delta=np.ascontiguousarray(t[1], F))
    return dict(count=n, reserved=0, index=None, delta=np.ascontiguousarray(t, F))


def _morph_entry(mesh, nv, targets):
    return dict(mesh=mesh, nv=nv, nt=len(targets), reserved=0, targets=[_target_entry(t, nv) for t in targets])


def skin_rules(skin, nv):
    """fovpt_set_skins' rules for one skin (joints, weights, joint count) of a mesh of nv vertices."""
    j, w, nj = np.asarray(skin[0]), np.asarray(skin[1], F), skin[2]
    return bool(j.shape == w.shape == (nv, 4) and 1 <= nj <= sk.MAX_JOINTS and (j < nj).all() and ((w >= 0) & (w <= 1)).all())


def test_the_verdict_on_seeded_skins_and_poses_is_the_restatements(driver):
    rng = np.random.default_rng(11)
    texts, want = [], []
    for seed in range(24):
        nv = int(rng.integers(1, 40))
        j, w, nj = sk.random_skin(rng, nv, int(rng.integers(1, 9)))
        if seed % 3 == 1:
            w[int(rng.integers(0, nv)), int(rng.integers(0, 4))] = rng.choice([np.nan, -0.25, 1.0, np.nextafter(F(1), F(2)), 0.0])
        if seed % 3 == 2:
            j[int(rng.integers(0, nv)), int(rng.integers(0, 4))] = nj + int(rng.integers(-1, 2))
        texts.append(skins_text(scene([5, nv]), [_skin_entry(1, nv, (j, w, nj))]))
        want.append(skin_rules((j, w, nj), nv))
    assert all(want[0::3]) and not all(want[1::3]) and any(want[1::3]) and not all(want[2::3]) and any(want[2::3])
    assert [a["code"] == 0 for a in driver(texts)] == want
    # palettes over large positions: skin_ref.accepted
    texts, want = [], []
    for k in range(50):
        nj = int(rng.integers(1, 6))
        pal = (rng.choice([-1.0, 1.0], (nj, 3, 4)) * 2.0 ** rng.uniform(15, 24.8, (nj, 3, 4))).astype(F)
        r = (rng.choice([-1.0, 1.0], (64, 3)) * 2.0 ** rng.uniform(90, 100, (64, 3))).astype(F)
        _, ww, _ = sk.random_skin(rng, 64, nj)
        if k % 2:
            ww[:] = 1
        texts.append(palette_text("fovpt_update_skinned", 0, nj, pal, sk.weight_sum(ww), absmax(r)))
        want.append(sk.accepted(r, ww, pal))
    assert 10 < sum(want) < 50
    assert [a["code"] == 0 for a in driver(texts)] == want


def test_the_verdict_on_seeded_targets_and_weights_is_morph_refs(driver):
    rng = np.random.default_rng(12)
    texts, want = [], []
    for k in range(60):
        r = (rng.choice([-1.0, 1.0], (32, 3)) * 2.0 ** rng.uniform(100, 126, (32, 3))).astype(F)
        ts = [(rng.choice([-1.0, 1.0], (32, 3)) * 2.0 ** rng.uniform(60, 100, (32, 3))).astype(F) for _ in range(6)]
        ws = (rng.choice([-1.0, 1.0], 6) * 2.0 ** rng.uniform(10, 25.5, 6)).astype(F)
        if k % 10 == 9:
            ws[int(rng.integers(0, 6))] = rng.choice([np.nan, np.inf])
        texts.append(weights_text(0, 6, ws, mr.target_max(ts, 32), absmax(r)))
        want.append(mr.accepted(r, ts, ws))
    assert 10 < sum(want) < 60
    answers = driver(texts)
    assert [a["code"] == 0 for a in answers] == want
    # seeded targets as fovpt_set_morphs takes them: accepted, and D is morph_ref.target_max
    for seed in range(8):
        nv = int(rng.integers(1, 50))
        ts = ac.shaped_targets(rng, nv, int(rng.integers(1, 8)))
        a = driver([morphs_text(scene([nv]), [_morph_entry(0, nv, ts)])])[0]
        assert a["code"] == 0 and np.array_equal(a["D0"], mr.target_max(ts, nv))


# ---- 4. accepted plans against the description itself ----------------------------------------------------------------------------------
def check_rig_plan(sc, d, a):
    nn, nmesh = d["num_nodes"], len(sc)
    at, blob = a["at"], a["blob"].astype(np.uint8)
    # the blob: 13 sections in order, 16-byte aligned, disjoint, inside; each holds its table
    sizes = [4 * nn, 4 * nn, 40 * nn, 4 * len(a["node_chan"]), 4 * len(a["w_chan"]), 4 * len(a["chan"]), 4 * len(a["times"]), 4 * len(a["values"]),
             4 * len(a["pal_node"]), 4 * len(a["pal_dst"]), 4 * len(a["inv_bind"]), 4 * len(a["rigid_node"]), 4 * len(a["wjobs"])]
    assert len(at) == 13 and all(o % 16 == 0 for o in at) and at[0] == 0
    assert all(at[k] + sizes[k] <= at[k + 1] < at[k] + sizes[k] + 16 for k in range(12)) and at[12] + sizes[12] == len(blob)
    for k, name in enumerate(("parent", "level", "rest", "node_chan", "w_chan", "chan", "times", "values", "pal_node", "pal_dst", "inv_bind", "rigid_node", "wjobs")):
        assert np.array_equal(blob[at[k]:at[k] + sizes[k]].view(np.uint32), a[name].astype(np.uint32)), name
    # nodes
    assert list(a["parent"]) == [N["parent"] for N in d["nodes"]]
    assert all(a["level"][i] == (0 if p < 0 else a["level"][p] + 1) for i, p in enumerate(a["parent"]))
    assert np.array_equal(a["rest"], np.concatenate([np.concatenate([N["translation"], N["rotation"], N["scale"]]) for N in d["nodes"]]).view(np.uint32))
    # bindings: the palette places are the skin's, the weights' places the morphs'
    bound = a["bound"].reshape(-1, 5)
    pal_node, pal_dst, rigid_node, wjobs, inv = [], [], [], [], []
    for B, row in zip(d["bindings"], bound):
        mesh = sc[B["mesh"]]
        assert list(row) == [B["mesh"], len(rigid_node) if B["node"] >= 0 else 0, B["num_joints"] != 0, mesh[3] != 0, B["node"] >= 0]
        pal_node += list(B["joint_nodes"][:B["num_joints"]]) if B["num_joints"] else []
        pal_dst += [mesh[2] + j for j in range(B["num_joints"])]
        inv += [B["inverse_bind"].reshape(-1)] if B["num_joints"] else []
        rigid_node += [B["node"]] if B["node"] >= 0 else []
        wjobs += [mesh[4], mesh[3]] if mesh[3] else []
    assert len(bound) == len(d["bindings"])
    assert list(a["pal_node"]) == pal_node and list(a["pal_dst"]) == pal_dst and list(a["rigid_node"]) == rigid_node and list(a["wjobs"]) == wjobs
    assert np.array_equal(a["inv_bind"], (np.concatenate(inv) if inv else np.zeros(0, F)).view(np.uint32))
    # channels: every channel's keys are in bounds and hold the inputs; the tables name exactly the channel that targets them
    chan = a["chan"].reshape(-1, 4)
    job_of = {wjobs[2 * k]: k for k in range(len(wjobs) // 2)}            # by the place of the weights
    node_chan, w_chan = np.full((d["num_clips"], 3 * nn), -1), np.full((d["num_clips"], len(wjobs) // 2), -1)
    h, t_next, v_next = 0, 0, 0
    for k, K in enumerate(d["clips"]):
        for H in K["channels"]:
            t_first, v_first, num_keys, interp = chan[h]
            width = sc[H["target"]][3] if H["path"] == rg.WEIGHTS else (4 if H["path"] == rg.ROTATION else 3)
            assert (t_first, v_first, num_keys, interp) == (t_next, v_next, H["num_keys"], H["interpolation"])
            assert t_first + num_keys <= len(a["times"]) and v_first + width * num_keys <= len(a["values"])
            assert np.array_equal(a["times"][t_first:t_first + num_keys], H["times"].view(np.uint32))
            assert np.array_equal(a["values"][v_first:v_first + width * num_keys], H["values"].reshape(-1).view(np.uint32))
            if H["path"] == rg.WEIGHTS:
                w_chan[k, job_of[sc[H["target"]][4]]] = h
            else:
                node_chan[k, 3 * H["target"] + H["path"]] = h
            h, t_next, v_next = h + 1, t_next + num_keys, v_next + width * num_keys
    assert h == len(chan) and t_next == len(a["times"]) and v_next == len(a["values"])
    assert np.array_equal(a["node_chan"], node_chan.reshape(-1)) and np.array_equal(a["w_chan"], w_chan.reshape(-1))
    # the scalars: levels, the floats k_rig_pose writes, and one workgroup's threads
    most = max([nn, len(pal_node)] + wjobs[1::2])
    threads = rg.MAX_NODES if most >= rg.MAX_NODES else (most + 63) // 64 * 64
    assert list(a["scalars"]) == [nn, d["num_clips"], max(a["level"]) + 1, threads, 12 * (nn + len(rigid_node) + len(pal_node))]


def test_accepted_rig_plans_are_the_description_laid_out(driver, rig_fixture):
    sc, _, _, _, plain = rig_fixture
    seeded = [(s, d) for s, sk_, mo, d in (_seeded_rig(seed) for seed in range(0, 36, 3))]
    big = rg.chain_rig(rg.MAX_NODES)                                      # the most nodes: one workgroup of 1024
    big["bindings"] = [dict(mesh=0, node=rg.MAX_NODES - 1)]
    rigs = [(sc, plain)] + seeded + [(scene([3]), ac.describe_rig(big)), (scene([3]), ac.describe_rig(rg.empty_rig(65)))]
    answers = driver([rig_text(s, d) for s, d in rigs])
    for (s, d), a in zip(rigs, answers):
        assert a["code"] == 0, a
        check_rig_plan(s, d, a)
    assert answers[-2]["scalars"][3] == 1024 and answers[-1]["scalars"][3] == 128 and answers[0]["scalars"][3] == 64


def test_accepted_morph_plans_are_the_targets_transposed(driver, base):
    morphs, skins = ac.morph_scene(base)
    nv = nv_of(base)
    # a scene whose mesh 1 has morphs already (2 targets, 7 entries): fovpt_set_morphs on meshes 3, 4 and 5 keeps them and lays all four out
    sc = scene(nv, {}, {1: (2, 7)})
    listed = [4, 5, 3]
    a = driver([morphs_text(sc, [_morph_entry(m, nv[m], morphs[m]) for m in listed])])[0]
    assert a["code"] == 0
    for k, m in enumerate(listed):
        split = [mr.split(t, nv[m]) for t in morphs[m]]
        count = np.zeros(nv[m], np.int64)
        for idx, _ in split:
            count[idx] += 1
        off, ent = a["off%d" % k], a["ent%d" % k].reshape(-1, 4)
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(count)])) and len(ent) == off[-1] == a["entries"][k]      # the running count per vertex
        for v in range(nv[m]):
            mine = ent[off[v]:off[v + 1]]
            assert (np.diff(mine[:, 3]) > 0).all()                        # within a vertex ascending by target
            for dx, dy, dz, t in mine:                                    # and the input's deltas
                idx, d = split[t]
                assert np.array_equal(as_floats([dx, dy, dz]), d[np.flatnonzero(idx == v)[0]])
        assert np.array_equal(a["D%d" % k], [np.abs(d.astype(np.float64)).max() if d.size else 0.0 for _, d in split])
    nt = {1: 2, **{m: len(morphs[m]) for m in listed}}
    ne = {1: 7, **{m: int(a["entries"][k]) for k, m in enumerate(listed)}}
    o = e = w = 0
    for m in range(len(nv)):
        assert (a["num_targets"][m], a["off_first"][m], a["ent_first"][m], a["w_first"][m]) == (nt.get(m, 0), o, e, w)
        if m in nt:
            o, e, w = o + nv[m] + 1, e + ne[m], w + nt[m]
    assert list(a["totals"]) == [o, e, w] and list(a["bytes"]) == [4 * o, 16 * e, 4 * w]
    # removing the last morphs leaves no buffers
    gone = driver([morphs_text(scene(nv, {}, {3: (1, nv[3])}), [dict(mesh=3, nv=nv[3], nt=0, reserved=0, targets=None)])])[0]
    assert gone["code"] == 0 and list(gone["totals"]) == [0, 0, 0] and list(gone["bytes"]) == [0, 0, 0]


def test_accepted_skin_plans_hold_the_weight_sums_and_the_places(driver, base):
    skins = ac.skin_scene(base)
    nv = nv_of(base)
    sc = scene(nv, {1: 2})                                                # mesh 1 has a skin of 2 joints already
    listed = [5, 3, 4]
    a = driver([skins_text(sc, [_skin_entry(m, nv[m], skins[m]) for m in listed])])[0]
    assert a["code"] == 0
    for k, m in enumerate(listed):
        w = skins[m][1].astype(np.float64)
        assert a["S"][k] == (((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]).max()           # the largest four-weight sum, in binary64
    assert list(a["S"]) == [1.0, 4.0, a["S"][2]]
    nj = {1: 2, **{m: skins[m][2] for m in listed}}
    first = pal = 0
    for m in range(len(nv)):
        assert (a["num_joints"][m], a["first"][m], a["pal_first"][m]) == (nj.get(m, 0), first, pal)
        if m in nj:
            first, pal = first + nv[m], pal + nj[m]
    assert list(a["totals"]) == [first, pal] and list(a["bytes"]) == [8 * first, 16 * first, 48 * pal]


# ---- 5. the 2^32 rules ------------------------------------------------------------------------------------------------------------------
def test_more_than_2_to_the_32_entries_are_refused(driver):
    """tests/test_morph_gpu.py's case of the same name, without its mesh: a scene view that claims one mesh of 2^24 vertices, and
    256 dense targets over one array of a few deltas.  The count is checked before any delta is read -- the array has six floats,
    and the sanitizer is the witness."""
    n = 1 << 24
    few = np.zeros((2, 3), F)

    def dense(nt):
        return [dict(mesh=1, nv=n, nt=nt, reserved=0, targets=[dict(count=n, reserved=0, index=None, delta=few)] * nt)]

    sc = scene([4, n])
    refused, counted = driver([morphs_text(sc, dense(256)), morphs_text(sc, dense(255), command="morph_counts")])
    assert refused["code"] == E_INVALID
    assert refused["text"] == "fovpt_set_morphs: more than 2^32 - 1 entries (%d) or offsets (%d)" % (256 * n, n + 1)
    assert counted["code"] == 0 and list(counted["totals"]) == [n + 1, 255 * n, 255] and list(counted["entries"]) == [255 * n]
    # the skinned vertices: a skin for a mesh of two vertices beside 256, or 255, skinned meshes of 2^24
    one = [_skin_entry(0, 2, (np.zeros((2, 4), np.uint16), np.full((2, 4), 0.25, F), 1))]
    a = driver([skins_text(scene([2] + [n] * k, {m: 1 for m in range(1, k + 1)}), one) for k in (256, 255)])
    assert a[0]["code"] == E_INVALID and a[0]["text"] == "fovpt_set_skins: more than 2^32 - 1 skinned vertices"
    assert a[1]["code"] == 0 and list(a[1]["totals"]) == [255 * n + 2, 256]


# ---- 6. the overflow rules on either side of 2^127 ------------------------------------------------------------------------------------
def test_overflow_rules_on_either_side_of_two_to_the_127(driver):
    """The inputs of test_transform_cpu.py, test_skin_cpu.py and test_morph_cpu.py's tests of the restatements' bounds: the
    header gives the restatements' verdicts."""
    texts, want = [], []
    # fovpt_update_transforms
    rest = np.array([[2.0 ** 100, 0, 0], [0, -(2.0 ** 99), 1.0]], F)      # A = 2^100
    ms = []
    m = np.zeros((3, 4), F)
    for m00, m01, m03 in ((2.0 ** 27, 0, 0), (np.nextafter(F(2.0 ** 27), F(np.inf)), 0, 0), (2.0 ** 26, -(2.0 ** 26), 0), (2.0 ** 26, -(2.0 ** 26), 2.0 ** 80)):
        m = np.zeros((3, 4), F)
        m[0, 0], m[0, 1], m[0, 3] = m00, m01, m03
        ms.append((rest, m))
    m = tf.IDENTITY.copy()
    m[2, 3] = F(2.0 ** 127)
    ms += [(rest, m), (np.zeros((0, 3), F), m)]
    for bad in (np.nan, np.inf, -np.inf):
        m = tf.IDENTITY.copy()
        m[1, 2] = bad
        ms.append((rest, m))
    texts += [transform_text(0, m, absmax(r)) for r, m in ms]
    want += [tf.accepted(r, m) for r, m in ms]
    assert want == [True, False, True, False, False, True, False, False, False]
    # fovpt_update_skinned
    for s, shift in ((1.0, 0), (4.0, 2)):
        w = np.zeros((2, 4), F)
        w[0, :int(s)] = 1
        w[1, 0] = 0.5
        pals = []
        for p100, p101, p103 in ((2.0 ** (27 - shift), 0, 0), (np.nextafter(F(2.0 ** (27 - shift)), F(np.inf)), 0, 0), (2.0 ** (26 - shift), -(2.0 ** (26 - shift)), 0),
                                 (2.0 ** (26 - shift), -(2.0 ** (26 - shift)), 2.0 ** 80)):
            pal = np.zeros((2, 3, 4), F)
            pal[1, 0, 0], pal[1, 0, 1], pal[1, 0, 3] = p100, p101, p103
            pals.append((rest, w, pal))
        pal = np.tile(tf.IDENTITY, (2, 1, 1))
        pal[0, 2, 3] = F(2.0 ** (127 - shift))
        pals += [(rest, w, pal), (np.zeros((0, 3), F), np.zeros((0, 4), F), pal)]
        small = np.array([[2.0 ** -40, 0, 0]], F)                         # A < 1: the entries of the blended matrix are bounded on their own
        pal = np.zeros((1, 3, 4), F)
        pal[0, 1, 2] = F(2.0 ** (127 - shift))
        pals.append((small, w[:1], pal.copy()))
        pal[0, 1, 2] = np.nextafter(pal[0, 1, 2], F(np.inf))
        pals.append((small, w[:1], pal))
        for bad in (np.nan, np.inf, -np.inf):
            pal = np.tile(tf.IDENTITY, (2, 1, 1))
            pal[1, 1, 2] = bad
            pals.append((rest, w, pal))
        texts += [palette_text("fovpt_update_skinned", 0, len(p), p, sk.weight_sum(ww), absmax(r)) for r, ww, p in pals]
        got = [sk.accepted(r, ww, p) for r, ww, p in pals]
        assert got == [True, False, True, False, False, True, True, False, False, False, False]
        want += got
    # fovpt_update_morphed: the weights' rule
    rest = np.array([[2.0 ** 126, 0, 0], [0, -(2.0 ** 100), 1.0]], F)    # A = 2^126
    targets = [np.array([[2.0 ** 100, 0, 0], [0, 0, -(2.0 ** 100)]], F), (np.array([0], np.uint32), np.array([[0, 2.0 ** 90, 0]], F))]
    w = F([2.0 ** 25, -(2.0 ** 35)])                                      # 2^126 + 2^125 + 2^125 = 2^127: not above
    ws = [w, F([-(2.0 ** 25), 2.0 ** 35])]
    for k in (0, 1):                                                      # one ulp more on either weight
        w2 = w.copy()
        w2[k] = np.nextafter(w[k], F(np.inf) * np.sign(w[k]))
        ws.append(w2)
    ws += [F([bad, 0.0]) for bad in (np.nan, np.inf, -np.inf)] + [F([0.0, bad]) for bad in (np.nan, np.inf, -np.inf)]
    texts += [weights_text(0, 2, x, mr.target_max(targets, 2), absmax(rest)) for x in ws]
    got = [mr.accepted(rest, targets, x) for x in ws]
    assert got == [True, True, False, False] + [False] * 6
    want += got
    # ... and a palette with B in A's place
    small, one, w4 = np.array([[2.0 ** -40, 0, 0]], F), F([1.0]), np.ones((1, 4), F)
    tiny, far, exact = [np.array([[2.0 ** -41, 0, 0]], F)], [np.array([[2.0 ** 100, 0, 0]], F)], [np.array([[2.0 ** 100 - 2.0 ** -40, 0, 0]], F)]
    zero = np.zeros((1, 3), F)

    def pal_of(e00, e03=0.0):
        p = np.zeros((1, 3, 4), F)
        p[0, 0, 0], p[0, 0, 3] = e00, e03
        return p

    both = [(small, tiny, one, pal_of(2.0 ** 127)), (small, far, one, pal_of(2.0 ** 26)), (small, far, F([0.0]), pal_of(2.0 ** 26)), (small, far, one, pal_of(2.0 ** 24)),
            (zero, exact, one, pal_of(2.0 ** 25)), (zero, exact, one, pal_of(2.0 ** 25, 2.0 ** 80))]
    for bad in (np.nan, np.inf, -np.inf):
        p = np.tile(tf.IDENTITY, (1, 1, 1))
        p[0, 1, 3] = bad
        both.append((small, tiny, one, p))
    got = [mr.accepted(r, t, x, w4, p) for r, t, x, p in both]
    assert got == [False, False, True, True, True, False, False, False, False]
    texts += [palette_text("fovpt_update_morphed", 0, 1, p, sk.weight_sum(w4), mr.bound(r, t, x)) for r, t, x, p in both]
    want += got
    assert [a["code"] == 0 for a in driver(texts)] == want
    # the norm rule of fovpt_set_rig: exactly 1/4 and exactly 4 are taken
    qs = [F([0, 0, 0, 0.5]), F([0, 2, 0, 0]), F([1, 1, 1, 1]), F([0, 0, 0, ac.below(0.5)]), F([ac.above(1.0), 1, 1, 1]), F([0, 0, 0, 0])]
    assert [a["code"] == 0 for a in driver(["norm " + vals(q, F) for q in qs])] == [rg.norm2_ok(q) for q in qs] == [True, True, True, False, False, False]
