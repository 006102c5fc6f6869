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
the late directed test 0.39 s; inside the whole suite the slowest were old seed 2 with 0.90 s and late seed 5 with 0.68 s.

The hdr family (af.script(seed, hdr=True), app_model.HdrModel; FOVPT_FUZZHDR_FROM / FOVPT_FUZZHDR_TO widen it) puts fovpt_variance,
fovpt_variance_filter, fovpt_bloom and fovpt_quality into the chain: post -> variance -> variance_filter -> focus -> bloom -> expose
-> quality -> packet -> warp | warp_motion | lens, every hand-over a device pointer into the stage before, with the operation
variance_reset and the refusals vfilter_no_image, variance_bad_config, bloom_bad_levels and quality_bad_ring (argument checks that
return before anything is enqueued).  The model keeps the moment history, the size of the context's own variance image, the rendered
frame's camera and the exposure state on the host and compares every stage bit for bit with variance_ref, bloom_ref and quality_ref,
always with the passes and gaze of the frame as rendered.  What a drawn frame happens to show (a history carried over a moved mesh, a
filter that changed pixels, a lit bloom level, an exposure taken from a state with steps, differing pixels under fovpt_quality) is
printed per seed and asserted over the default seeds together.  Its directed case: the tall block of the Cornell box moved between
two moment steps. Time, in one run of this module on an MI355X: the hdr seeds 0.14 ... 0.91 s (seed 5, an atrium at 96 x 64 with
five chains; seed 2: 0.82 s, seeds 7 and 3 at 192 x 128: 0.69 and 0.64 s), the late seeds of the same run 0.06 ... 0.69 s (seed 2)
and the old ones 0.05 ... 0.72 s behind the process's first test, test_moments_follow_a_moved_block 0.10 s, the summary test
nothing it has not run already; three times the slowest late seed is 2.1 s, and no new test comes near it.  Inside the whole suite
the slowest were hdr seed 5 with 0.91 s and hdr seed 2 with 0.84 s, beside late seed 2 with 0.73 s.  As the only test of a
process an hdr seed takes 3.7 ... 4.7 s, the directed test 12 s, start-up included."""
import numpy as np
import pytest

import app_fuzz as af
import post_ref as po
import skin_ref as sk
import morph_ref as mr
import transform_ref as tf
from fovpathtracing_optixcodelatest_amd import scenes

from app_model import AppModel, LateModel, with_pytest_code
from gpu_common import bits

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


# ---- the hdr family ----------------------------------------------------------------------------------------------------------------
HDR_LOGS = {}                                            # seed -> (script, the model's log)


def _hdr(oracle, seed):
    """Runs an hdr seed once per process; a run that raised is remembered and raises again from the record (see _late)."""
    from app_model import HdrModel
    if seed not in HDR_LOGS:
        HDR_LOGS[seed] = None
        s = af.script(seed, hdr=True)
        model, cam = af.scene_of(s)
        m = HdrModel(oracle, s, model, cam, PROBE)
        try:
            m.run()
            HDR_LOGS[seed] = (s, m.log)
        except Exception as e:
            HDR_LOGS[seed] = e
            raise
        finally:
            m.close()
    got = HDR_LOGS[seed]
    if got is None or isinstance(got, Exception):
        raise AssertionError("hdr seed %d has failed in this process already, it is not run again: %r" % (seed, got))
    return got


HDR_STAGES = ("variance", "vfilter", "bloom", "quality")


def _hdr_conditions(logs):
    """What keeps the sweep from being vacuous, on the models' logs -> {condition: met}.  A variance entry is ("variance",
    had_history, spatial_count, kept_count, reject_depth, reject_class, moved, pixels)."""
    v = [x for x in logs if x[0] == "variance"]
    return {
        "a variance step with a history over a moved mesh: pixels kept, taps rejected, the window on some pixels and not on all":
            any(x[1] and x[6] and x[3] > 0 and x[4] + x[5] > 0 and 0 < x[2] < x[7] for x in v),
        "a filter changed pixels": any(x[0] == "vfilter" and x[1] > 0 for x in logs),
        "a bloom lit level 0": any(x[0] == "bloom" and x[3] > 0 for x in logs),
        "a bloom took the exposure of a state with steps": any(x[0] == "bloom" and x[2] for x in logs),
        "a quality measurement saw differing pixels": any(x[0] == "quality" and x[2] > 0 for x in logs),
    }


@pytest.mark.parametrize("seed", af.HDR_SEEDS)
def test_random_hdr_application(oracle, seed):
    """An hdr script on one context (app_model.HdrModel compares every stage of every chain bit for bit with its restatement, the
    state on the host): every chain entry of the script left exactly one log entry (the refusals are operations of their own and
    leave none).  The conditions against vacuity depend on what a drawn frame shows; they are printed here for every seed and
    asserted over the default seeds together (test_the_hdr_default_seeds_together)."""
    s, log = _hdr(oracle, seed)
    chains = [o["chain"] for o in s["ops"] if o["op"] == "frame"]
    print("hdr seed %d:" % seed, [x for x in log if x[0] in HDR_STAGES + ("adopt", "race")])
    print("hdr seed %d:" % seed, _hdr_conditions(log))
    for stage in HDR_STAGES:
        assert len([x for x in log if x[0] == stage]) == sum(c[stage] is not None for c in chains), stage
    assert len([x for x in log if x[0] == "post"]) >= 2


def test_the_hdr_default_seeds_together(oracle):
    logs = [x for seed in af.HDR_DEFAULT_SEEDS for x in _hdr(oracle, seed)[1]]
    missed = [k for k, met in _hdr_conditions(logs).items() if not met]
    assert not missed, missed


def test_moments_follow_a_moved_block(oracle):
    """On the Cornell box at 64 x 45, three tracked steps, each followed by fovpt_variance with the step's motion vectors and
    G-buffer; then the tall block (mesh 4) is moved sideways by fovpt_update_transforms and a fourth frame, step and variance call
    follow.  On the restatement (which the device equals bit for bit: HdrModel.variance): the block's pixels carry their history
    along by the block's own motion, the pixels it uncovered start again and take the window, taps are rejected by depth.  The
    restatement with no motion and with the interval before's motion each differ from the device on the block: the test can tell.
    Then fovpt_variance_reset ends the history; fovpt_temporal_reset does not: a call with motion = NULL behind it continues the
    history (and differs from the restatement without one), while the step's own motion is w = 0 everywhere and starts every pixel
    again."""
    import variance_ref as vr
    from app_model import HdrModel
    model = scenes.cornell_box()
    s = dict(seed="directed-hdr", size=(64, 45), ops=[], late=True, hdr=True, skins={}, morphs={}, rig=None,
             config=dict(uniform=0, r_inner=8, r_outer=18, spp=(1, 2, 4, 1), max_depth=2, frames_in_flight=0, chains_per_frame=0),
             post=dict(temporal=dict(history_fovea=3, history_middle=5, history_periphery=8, history_uniform=6)))
    m = HdrModel(oracle, s, model, scenes.CORNELL_CAMERA, PROBE)
    r = m.r
    stages = po.RECONSTRUCT | po.TEMPORAL | po.MOTION
    cfg = dict(vr.MOMENT_DEFAULTS, spatial_below=2)
    vd = dict(cfg=cfg, gbuffer="temporal", motion=True, own=True, adopt=False)
    view = dict(gaze=(28, 20), subframe_index=0, eye=(0.0, 0.0, 0.0))
    chain = dict(post=stages, variance=vd, vfilter=None, focus=None, bloom=None, expose=None, quality=None, packet=False, codec=None, last=None)
    frame = dict(op="frame", views=[view], between=[], pre_chain=None, chain=chain, sync=True, moved_on=None)

    def on_block(gb):
        prim = gb["prim"]
        return (prim != 0xffffffff) & (m.mesh_of_prim[np.where(prim == 0xffffffff, 0, prim).astype(np.int64)] == 4)

    def one(motion_of=None):
        """A frame, a step and a variance call -> (step output, history before, history after, the restatement's record)."""
        m.frames(frame)
        out = m.step(stages=stages)
        before = m.var_prev
        m.variance(vd, out["motion"], r.motion_buffer())
        rec = {}
        hist, _ = vr.moments(before, r.downloadAccum(), out["gb"], m.cam_rendered, m.rendered_fills()[0], out["motion"], cfg, rec)
        assert np.array_equal(bits(hist), bits(m.var_prev))
        return out, before, hist, rec
    try:
        for _ in range(2):
            m.run_op(frame)
        out3, _, hist3, _ = one()
        assert (hist3[..., 2] == 3).mean() > 0.9                             # a static scene: three steps of history
        was = on_block(out3["gb"])
        m.update({4: tf.rotation_translation(0.0, (368.0, 0.0, 351.0), (-45.0, 0.0, 0.0))}, kind="transforms")
        out, before, hist, rec = one()
        now = on_block(out["gb"])
        n, mv = hist[..., 2], out["motion"]
        back = now & (mv[..., 3] == 1)
        assert now.sum() > 60 and back.sum() > 30 and (np.abs(mv[back][:, 0]) > 2.0).mean() > 0.9      # several pixels, by its own motion
        # the block took its history along: of its 174 pixels the restatement keeps one on 139 (the rest are its leading edge,
        # which lands on what was wall a frame ago and is rejected by depth, and the pixels whose landing lies outside the block)
        assert (n[back] >= 2).sum() > 120 and (n[back] >= 2).mean() > 0.75
        # what it uncovered starts again and takes the window: 39 of 41 pixels (two at its foot land within the depth tolerance
        # of the floor beside it)
        gone = was & ~now
        assert gone.sum() > 30 and (n[gone] == 1).mean() > 0.9 and rec["spatial"][gone & (n == 1)].all()
        assert rec["reject_depth"].sum() > 0 and rec["reject_depth"][gone].sum() > 0
        print("moved block: %d pixels on it, %d with a history, %d uncovered, %d of them new; taps rejected by depth %d, by class %d"
              % (now.sum(), (n[back] >= 2).sum(), gone.sum(), (n[gone] == 1).sum(), rec["reject_depth"].sum(), rec["reject_class"].sum()))
        for label, other in (("no motion", None), ("the interval before's motion", out3["motion"])):
            leak, _ = vr.moments(before, r.downloadAccum(), out["gb"], m.cam_rendered, m.rendered_fills()[0], other, cfg)
            assert not np.array_equal(bits(leak[now]), bits(hist[now])), label
        r.variance_reset()
        m.var_prev = None
        _, _, hist, _ = one()
        assert (hist[..., 2] == 1).all()
        one()
        # fovpt_temporal_reset leaves the moments.  Read at the pixel itself (motion = NULL) the history of two steps goes on to
        # three: a moment history that ended with the temporal one would give n == 1, which the restatement without a history shows
        r.temporal_reset()
        m.reset()
        m.frames(frame)
        out = m.step(stages=stages)
        assert (out["motion"][..., 3] == 0).all()
        before = m.var_prev
        assert before is not None and (before[..., 2] == 2).mean() > 0.9
        m.variance(dict(vd, motion=False), None, None)                       # (asserts device == restatement on the model's history)
        hist = m.var_prev
        assert np.array_equal(hist[..., 2], before[..., 2] + 1) and (hist[..., 2] == 3).mean() > 0.9      # a static scene: every pixel goes on
        ended, _ = vr.moments(None, r.downloadAccum(), out["gb"], m.cam_rendered, m.rendered_fills()[0], None, cfg)
        assert (ended[..., 2] == 1).all() and not np.array_equal(bits(ended), bits(hist))
        # ... and the step right behind a temporal reset says of no pixel where it was (w = 0): with that motion the restatement
        # starts every pixel again, on moments that are still there
        r.temporal_reset()
        m.reset()
        out, before, hist, _ = one()
        assert before is not None and (out["motion"][..., 3] == 0).all() and (hist[..., 2] == 1).all()
        print("after temporal_reset, motion with w = 0: n == 1 on %d of %d pixels" % ((hist[..., 2] == 1).sum(), hist[..., 2].size))
    finally:
        m.close()
