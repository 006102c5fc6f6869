"""A seeded fuzz of an animated application's whole frame loop: tests/app_fuzz.py draws a scene, a frame size, a render config,
skins, morph targets and ten operations -- updates of all four kinds (host and device, refit and rebuild), skin and morph
registration, one to three frames (also in flight, with updates and refused calls between them), the post chain (fovpt_post,
fovpt_expose, fovpt_packet_*), resizes, scene reloads, resets, refused calls -- and tests/app_model.py runs them on one context,
checking after every operation what it defines against the restatements of tests/*_ref.py, the CPU oracle and a twin context.
tests/test_app_fuzz_cpu.py holds the generator to what the sweep is there for.  FOVPT_FUZZAPP_FROM / FOVPT_FUZZAPP_TO widen it.

Beside it the directed case the sweep reaches only by chance: one mesh moved by all four kinds in one temporal interval.

The late family (af.script(seed, late=True), app_model.LateModel; FOVPT_FUZZLATE_FROM / FOVPT_FUZZLATE_TO widen it) drives what came
after: fovpt_set_rig / fovpt_update_animated, FOVPT_UPDATE_REBUILD_ASYNC with fovpt_rebuild_state, fovpt_focus, fovpt_warp,
fovpt_warp_motion, fovpt_lens and coded packets, in the chain post -> focus -> expose -> packet -> warp | warp_motion | lens, with
the refusals no_rig, clip_range, async_with_rebuild and warp_motion_stale; tests/test_app_fuzz_cpu.py lists the operations and
situations the eight default seeds hold.  Background builds stay deterministic: no pixel depends on the tree in use; an update that
may adopt runs after rebuild_state(WAIT), or the model reads fovpt_rebuild_state(0).adopted once after it, accepts "not adopted"
and "adopted by one" and goes on with what happened (the outcomes are printed, never asserted); nothing sleeps, and the one script
that sets FOVPT_ASYNC_BUILD_DELAY_MS (150 ms, seed 1) does it to make it likely that two updates meet the build still running,
so that the adoption refits a stale snapshot; no assertion depends on whether they did (it is printed).  Its directed case: an adoption between a temporal step and the fovpt_warp_motion that uses the step's G-buffer.

Time, measured on an MI355X: a default seed takes 0.6 ... 0.7 s inside a running suite and 3.6 ... 4.4 s (seed 2, an atrium)
as the only test of a process, where it also pays for loading the library, the oracle and torch; the directed test less than
3.6 s inside the suite.  The restatements' share is small: post_ref.post with every stage takes 0.05 s at 127 x 41 and 0.21 s at
192 x 128 on the CPU.  The late seeds and the old ones in one run of this module on an MI355X (the first test of the process
carries 12 s of start-up): old seeds 0.04 ... 0.82 s (seed 2), late seeds 0.06 ... 0.76 s (seed 2, an atrium; seed 5: 0.68 s),
the late directed test 0.39 s; inside the whole suite the slowest were old seed 2 with 0.90 s and late seed 5 with 0.68 s."""
import numpy as np
import pytest

import app_fuzz as af
import post_ref as po
import skin_ref as sk
import morph_ref as mr
import transform_ref as tf
from fovpathtracing_optixcodelatest_amd import scenes

from app_model import AppModel, LateModel, with_pytest_code
from postprocess_common import bits

pytestmark = pytest.mark.gpu
PROBE = scenes.ambient_probe(64, 32, 2.0)
F = np.float32


@pytest.mark.parametrize("seed", af.SEEDS)
def test_random_application(oracle, seed):
    s = af.script(seed)
    model, cam = af.scene_of(s)
    m = AppModel(oracle, s, model, cam, PROBE)
    try:
        m.run()
        posts = [x for x in m.log if x[0] == "post"]
        assert len(posts) >= 2 and any(had for _, _, had in posts)          # (some step did reproject a history)
        trees = [agreed for what, agreed in (x for x in m.log if x[0] == "tree")]
        assert 2 * sum(trees) >= len(trees), trees                          # (the twin's tree was mostly compared entry for entry)
    finally:
        m.close()


def test_every_kind_twice_in_one_interval(oracle):
    """On the Cornell box, after two tracked steps: the tall block (mesh 4) is moved by fovpt_update_vertices, _transforms,
    _skinned and _morphed in turn, the last with a rebuild, the short block (3) by two of them, all within one interval.  The
    next step's motion vectors are post_ref's from the positions at the previous step to the last ones; no intermediate
    position leaks in (the restatement over any of them differs), and the previous positions the library keeps for the marked
    meshes are those of the previous step after every one of the updates (AppModel.check_scene)."""
    model = scenes.cornell_box()
    rng = np.random.default_rng(5)
    v3, v4 = model.meshes[3].vertex, model.meshes[4].vertex
    s = dict(seed="directed", size=(64, 45), ops=[],
             config=dict(uniform=0, r_inner=8, r_outer=18, spp=(1, 2, 4, 1), max_depth=2, frames_in_flight=0, chains_per_frame=0),
             post=dict(temporal=dict(history_fovea=3, history_middle=5, history_periphery=8, history_uniform=6)),
             skins={3: sk.bend(v3, 2), 4: sk.bend(v4, 3)}, morphs={4: mr.bumps(v4, 2, 1, fraction=0.3, height=25.0)})
    m = AppModel(oracle, s, model, scenes.CORNELL_CAMERA, PROBE)
    stages = po.RECONSTRUCT | po.TEMPORAL | po.MOTION
    view = dict(gaze=(28, 20), subframe_index=0, eye=(0.0, 0.0, 0.0))
    frame = dict(op="frame", views=[view], between=[], pre_chain=None, chain=dict(post=stages, expose=None, packet=False), sync=True)
    try:
        for _ in range(2):
            m.run_op(frame)
        assert m.tracking and m.prev is not None
        start = m.vtx.copy()
        between = []
        m.update({4: (v4 + F([30, 0, -20])).astype(F)}, kind="vertices")
        between.append(m.vtx.copy())
        m.update({4: tf.rotation_translation(15.0, (368.0, 0.0, 351.0), (-60.0, 0.0, 10.0)), 3: tf.scale_about((186.0, 0.0, 168.0), (1.2, 0.7, 1.0))}, kind="transforms")
        between.append(m.vtx.copy())
        m.update({4: sk.bend_pose(v4, 3, 30.0, (-25.0, 0.0, -15.0)), 3: sk.bend_pose(v3, 2, -20.0, (15.0, 0.0, 0.0))}, kind="skinned", device=True)
        between.append(m.vtx.copy())
        m.update({4: (F([1.0, -0.5, 0.75]), sk.bend_pose(v4, 3, -12.0, (-40.0, 0.0, 25.0)))}, kind="morphed", rebuild=True)
        assert np.array_equal(bits(m.vtx_step), bits(start)) and m.moved[[3, 4]].all() and m.moved.sum() == 2
        prev, motion = m.prev, m.motion()
        m.frames(frame)
        out = m.step(stages=stages)                                          # (asserts colour, history and motion against post_ref)
        prim = out["gb"]["prim"]
        on4 = (prim != 0xffffffff) & (m.mesh_of_prim[np.where(prim == 0xffffffff, 0, prim).astype(np.int64)] == 4)
        mv = out["motion"][on4]
        back = mv[:, 3] == 1                                                 # the block's pixels that reproject
        assert on4.sum() > 60 and back.sum() > 30 and (out["history"][on4][:, 3] > 1).any()
        assert (mv[back][:, :2] != 0).any(axis=-1).mean() > 0.9              # ... by the block's own motion: the camera stood still
        for k, mid in enumerate(between):                                    # the test can tell: an intermediate position would show
            leak = po.post(stages, out["frame"], prev, s["post"], dict(motion, vtx_prev=mid))["motion"]
            assert not np.array_equal(bits(leak[on4]), bits(out["motion"][on4])), k
    finally:
        m.close()


# ---- the late family ---------------------------------------------------------------------------------------------------------------
LATE_LOGS = {}                                           # seed -> the model's log, for the summary over the default seeds


def _late(oracle, seed):
    """Runs a late seed once per process.  A run that raised is remembered too and raises again from the record: what failed
    (or faulted) is never started a second time by the summary test."""
    if seed not in LATE_LOGS:
        LATE_LOGS[seed] = None                           # (an error below, of any kind, leaves this behind)
        s = af.script(seed, late=True)
        model, cam = af.scene_of(s)
        m = LateModel(oracle, s, model, cam, PROBE)
        try:
            m.run()
            LATE_LOGS[seed] = (s, m.log)
        except Exception as e:
            LATE_LOGS[seed] = e
            raise
        finally:
            m.close()
    got = LATE_LOGS[seed]
    if got is None or isinstance(got, Exception):
        raise AssertionError("late seed %d has failed in this process already, it is not run again: %r" % (seed, got))
    return got


@pytest.mark.parametrize("seed", af.LATE_SEEDS)
def test_random_late_application(oracle, seed):
    """A late script on one context (app_model.LateModel checks every operation), then what keeps the run from being vacuous,
    on the model's log and the restatements' outputs, where the script holds the operation.  A lens step changes the image in
    every script (the defaults' polynomial moves every pixel off the axis).  The other three conditions are on what a drawn frame
    happens to show, and a drawn script may miss them for no fault of the library's: the mesh of the interval's updates is hidden
    or outside the frame (one of 103 in the atrium), or moves less than half a pixel, so that no pixel lands elsewhere than under
    fovpt_warp; every depth under a drawn strength and cap stays below a blur radius of 0.5, so that fovpt_focus copies; a
    level's blocks are each of one colour (the 3 x 50 frame has no packet at all).  They are asserted for the default seeds, whose
    scripts tests/test_app_fuzz_cpu.py pins and which were seen to meet them, and printed for a widened sweep."""
    s, log = _late(oracle, seed)
    default = seed in af.LATE_DEFAULT_SEEDS
    chains = [o["chain"] for o in s["ops"] if o["op"] == "frame"]
    moving = [x for x in log if x[0] == "warp_motion" and x[1]]
    focus = [x for x in log if x[0] == "focus"]
    lens = [x for x in log if x[0] == "lens"]
    coded = [x for x in log if x[0] == "coded" and x[1] is not None and af.BC1 in x[1]]
    print("late seed %d:" % seed, [x for x in log if x[0] in ("race", "adopt", "stale", "warp_motion", "focus", "lens", "coded")])
    assert len([x for x in log if x[0] == "post"]) >= 2
    assert len(focus) == sum(c["focus"] is not None for c in chains) and len(lens) == sum(c["last"] is not None and c["last"]["stage"] == "lens" for c in chains)
    assert all(x[1] for x in lens), "a lens step left the image as it was"
    if default:
        assert not moving or any(x[2] for x in moving), "no warp_motion with a moved mesh differs from fovpt_warp"
        assert not focus or any(x[3] > 0 for x in focus), "no focus step acted on a pixel"
        assert not coded or any(x[2] > 0 for x in coded), "no BC1 block with two different endpoints"
    for x in log:
        if x[0] == "warp_motion" and not x[1]:
            assert not x[2]                                                  # (nothing known to move: fovpt_warp's bits)
    stale = [x[1] for x in log if x[0] == "stale"]
    assert stale == ["refused", "accepted"] * (len(stale) // 2)


def test_the_late_default_seeds_together(oracle):
    """Over the eight default seeds (run here if the sweep above was not): an AUTO focus step metered something, a warp_motion
    moved a mesh, an adoption happened and its tree was compared entry for entry with the twin's.  The outcomes of the races (an
    update or rebuild_state(ADOPT) issued without a wait before it) are printed, not asserted, and so is what depends on them:
    whether some adoption took a snapshot older than the positions it was refitted to, which needs an update that met the build
    still running (seed 1 is written for it, and holds the builder back 150 ms to make it likely; nothing can make it certain)."""
    logs = [x for seed in af.LATE_DEFAULT_SEEDS for x in _late(oracle, seed)[1]]
    assert any(x[0] == "focus" and x[1] == af.AUTO and x[2] for x in logs)
    assert any(x[0] == "warp_motion" and x[1] and x[2] for x in logs)
    assert any(x[0] == "warp_motion" and x[3] for x in logs)                # a step that did not know the motion
    adopted = [x for x in logs if x[0] == "adopt"]
    assert adopted and any(x[4] is True for x in adopted), adopted
    races = [x[1:] for x in logs if x[0] == "race"]
    print("races (where, adopted):", races)
    print("adoptions (by, snapshot_update, updates before): %s; a snapshot older than the positions at its adoption: %s"
          % ([x[1:4] for x in adopted], any(x[2] < x[3] for x in adopted)))


def test_an_adoption_between_a_step_and_its_warp(oracle):
    """On the Cornell box at 64 x 45, after two tracked steps: fovpt_update_animated with FOVPT_UPDATE_REBUILD_ASYNC, a frame with
    post(MOTION), fovpt_temporal_gbuffer, fovpt_rebuild_state(WAIT | ADOPT).  The adoption makes the step's G-buffer stale for
    fovpt_warp_motion (FOVPT_E_NO_FRAME) and leaves everything else as it was: with its own trace the warp is the restatement's
    with the animated meshes' motion, and the next steps' motion vectors and histories are post_ref's from the model's own
    previous positions, which know nothing of the adoption."""
    from test_rig_gpu import cornell_rig, cornell_skins
    model = scenes.cornell_box()
    s = dict(seed="directed-late", size=(64, 45), ops=[], late=True,
             config=dict(uniform=0, r_inner=8, r_outer=18, spp=(1, 2, 4, 1), max_depth=2, frames_in_flight=0, chains_per_frame=0),
             post=dict(temporal=dict(history_fovea=3, history_middle=5, history_periphery=8, history_uniform=6)),
             skins=cornell_skins(model), morphs={}, rig=cornell_rig(model))
    m = LateModel(oracle, s, model, scenes.CORNELL_CAMERA, PROBE)
    r = m.r
    stages = po.RECONSTRUCT | po.TEMPORAL | po.MOTION
    view = dict(gaze=(28, 20), subframe_index=0, eye=(0.0, 0.0, 0.0))
    frame = dict(op="frame", views=[view], between=[], pre_chain=None, chain=dict(post=stages, expose=None, packet=False), sync=True)
    eye = tuple(float(x) for x in np.asarray(scenes.CORNELL_CAMERA["eye"], np.float64) + np.array([6.0, 2.0, 0.0]))
    la = dict(stage="warp_motion", to=("slide", eye, scenes.CORNELL_CAMERA["lookat"]), images=3, fill_radius=2, advance=1.0, gbuffer="own", adopt=False)
    try:
        for _ in range(2):
            m.run_op(frame)
        m.update(dict(clip=0, time=0.75), rebuild="async", kind="animated")
        assert m.rec["flight"] and m.moved[[3, 4]].all() and m.moved.sum() == 2
        m.frames(frame)
        m.step(stages=stages)
        g = r.temporal_gbuffer()
        updates = m.updates
        m.rebuild_state(True, True)
        assert m.updates == updates + 1 and m.rec["adopted"] == 1 and not m.rec["flight"]
        with_pytest_code(af.E_NO_FRAME, lambda: r.warp_motion(m.to_camera(la["to"])[0], None, g))
        m.warp(la, None, None, m.last_rgba, None)
        assert m.log[-1] == ("warp_motion", True, True, False), m.log[-1]   # the blocks go on moving: not fovpt_warp's image
        m.frames(frame)
        out = m.step(stages=stages)                                          # (asserts colour, history and motion against post_ref)
        assert (out["history"][..., 3] > 1).mean() > 0.3                     # the history went on across the adoption
        m.update(dict(clip=0, time=1.5), kind="animated")
        m.frames(frame)
        out = m.step(stages=stages)
        prim = out["gb"]["prim"]
        on4 = (prim != 0xffffffff) & (m.mesh_of_prim[np.where(prim == 0xffffffff, 0, prim).astype(np.int64)] == 4)
        assert on4.sum() > 60 and (out["motion"][on4][:, :2] != 0).any()     # the tall block's own motion, from tracked positions
        m.check_info()
    finally:
        m.close()
