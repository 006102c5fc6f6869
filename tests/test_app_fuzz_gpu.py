"""A seeded fuzz of an animated application's whole frame loop: tests/app_fuzz.py draws a scene, a frame size, a render config,
skins, morph targets and ten operations -- updates of all four kinds (host and device, refit and rebuild), skin and morph
registration, one to three frames (also in flight, with updates and refused calls between them), the post chain (fovpt_post,
fovpt_expose, fovpt_packet_*), resizes, scene reloads, resets, refused calls -- and tests/app_model.py runs them on one context,
checking after every operation what it defines against the restatements of tests/*_ref.py, the CPU oracle and a twin context.
tests/test_app_fuzz_cpu.py holds the generator to what the sweep is there for.  FOVPT_FUZZAPP_FROM / FOVPT_FUZZAPP_TO widen it.

Beside it the directed case the sweep reaches only by chance: one mesh moved by all four kinds in one temporal interval.

Time, measured on an MI355X: a default seed takes 0.6 ... 0.7 s inside a running suite and 3.6 ... 4.4 s (seed 2, an atrium)
as the only test of a process, where it also pays for loading the library, the oracle and torch; the directed test less than
3.6 s inside the suite.  The restatements' share is small: post_ref.post with every stage takes 0.05 s at 127 x 41 and 0.21 s at
192 x 128 on the CPU."""
import numpy as np
import pytest

import app_fuzz as af
import post_ref as po
import skin_ref as sk
import morph_ref as mr
import transform_ref as tf
from fovpathtracing_optixcodelatest_amd import scenes

from app_model import AppModel
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
