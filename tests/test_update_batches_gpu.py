"""The edges of the update calls' shared host steps (csrc/api_animate.hip): batches of FOVPT_GATHER_BATCH = 32 meshes per launch
and host data staged with runs of neighbouring meshes in one copy.  A scene of 66 one-triangle meshes, each with a two-joint skin
and two morph targets (one dense, one sparse), is updated through every source -- host and device vertices, transforms, host and
device palettes, host and device weights without and with palettes -- with lists of 1, 32, 33, 64 and 66 meshes, every second
mesh (no two staged runs are neighbours) and meshes 0-9 and 20-29 (two runs of ten); morph poses with palettes on an irregular
subset, so that the two batches of that call fill at different times; and, with fovpt_temporal_motion's tracking on, lists whose
first-touched meshes fill a batch, leave one partly full behind an already marked last mesh, and are none at all.  After every
call the library's status is clean, the device positions ("scene_vertices", and "scene_vertices_prev" of the marked meshes) are
the numpy restatements' bit for bit, and a 16 x 16 frame renders."""
import numpy as np
import pytest

import morph_ref as mr
import skin_ref as sk
import transform_ref as tf
from fovpathtracing_optixcodelatest_amd import scenes

from common import cfg_foveated, make_gpu
from gpu_common import bits, debug_buffer
from temporal_common import tcfg

pytestmark = pytest.mark.gpu
F = np.float32
NMESH, BATCH = 66, 32
SIZE = (16, 16)
CAMERA = dict(eye=(5.0, 2.5, 14.0), lookat=(5.0, 2.5, 0.0), up=(0.0, 1.0, 0.0), fovy=50.0)
PROBE = scenes.ambient_probe(32, 16, 2.0)
LISTS = {"1": [40], "32": list(range(32)), "33": list(range(33)), "64": list(range(1, 65)), "66": list(range(NMESH)),
         "every_second": list(range(0, NMESH, 2)), "two_runs_of_ten": list(range(10)) + list(range(20, 30))}
SOURCES = ("vertices_host", "vertices_device", "transforms", "skinned_host", "skinned_device", "morphed_host", "morphed_device",
           "morphed_skinned_host", "morphed_skinned_device")


def build_model():
    """66 triangles in an 11 x 6 grid facing the camera, three vertices per mesh."""
    material = scenes.cornell_box().meshes[1].material
    rng = np.random.default_rng(66)
    meshes = []
    for k in range(NMESH):
        corner = np.array([k % 11, k // 11, 0.0]) + rng.uniform(-0.05, 0.05, 3)
        v = (corner + np.array([[0.0, 0.0, 0.0], [0.8, 0.0, 0.1], [0.1, 0.8, 0.2]])).astype(F)
        meshes.append(scenes.TriangleMesh(v, np.array([[0, 1, 2]], np.uint32), material, np.zeros((3, 2), F), -1))
    return scenes.Model(meshes)


class Scene:
    """A renderer over the model with its skins and morphs set, and the positions its device buffer must hold."""

    def __init__(self, tracking=False):
        self.model = build_model()
        rng = np.random.default_rng(7)
        self.skins = {k: sk.random_skin(rng, 3, 2) for k in range(NMESH)}
        self.morphs = {k: [rng.uniform(-0.3, 0.3, (3, 3)).astype(F), (np.array([1 + k % 2], np.uint32), rng.uniform(-0.3, 0.3, (1, 3)).astype(F))]
                       for k in range(NMESH)}
        cfg = cfg_foveated(3, 6, (1, 1, 2))
        cfg.write_guides = 1
        self.r = make_gpu(self.model, PROBE, CAMERA, SIZE, cfg)
        self.r.set_skins(self.skins)
        self.r.set_morphs(self.morphs)
        self.vtx = np.concatenate([m.vertex for m in self.model.meshes])
        self.calls = 0
        self.tracking = tracking
        self.marked, self.vtx_step = set(), self.vtx.copy()
        if tracking:
            self.step()

    def step(self):
        """A frame and a fovpt_temporal_motion step: the first switches tracking on, each ends the interval of the marks."""
        self.r.launchParams.frame.subframe_index = 0
        self.r.render()
        self.r.temporal_motion(tcfg(None))
        self.marked, self.vtx_step = set(), self.vtx.copy()

    def update(self, source, meshes, with_palette=None):
        """One call of `source` over `meshes` with values of its own, then the checks.  with_palette: the meshes of a morphed
        call that carry a palette (default: all of them for the morphed_skinned sources, none otherwise)."""
        import torch
        self.calls += 1
        rng = np.random.default_rng(1000 + self.calls)
        model, r = self.model, self.r
        device = source.endswith("_device")

        def dev(x):
            return tuple(dev(y) for y in x) if isinstance(x, tuple) else torch.from_numpy(np.ascontiguousarray(x, F)).cuda()

        rest = {k: model.meshes[k].vertex for k in meshes}
        if source.startswith("vertices"):
            give = new = {k: (rest[k] + rng.uniform(-0.2, 0.2, (3, 3))).astype(F) for k in meshes}
            call = r.update_vertices
        elif source == "transforms":
            give = {k: tf.rotation_translation(rng.uniform(-30, 30), rest[k].mean(axis=0), rng.uniform(-0.2, 0.2, 3)) for k in meshes}
            new, call = tf.restate(model, give), r.update_transforms
        elif source.startswith("skinned"):
            give = {k: sk.random_pose(rng, rest[k], 2) for k in meshes}
            new, call = sk.restate(model, self.skins, give), r.update_skinned
        else:
            if with_palette is None:
                with_palette = meshes if source.startswith("morphed_skinned") else []
            weights = {k: rng.uniform(0.25, 1.5, 2).astype(F) for k in meshes}
            give = {k: ((weights[k], sk.random_pose(rng, rest[k], 2)) if k in with_palette else weights[k]) for k in meshes}
            new, call = mr.restate(model, self.morphs, give, self.skins), r.update_morphed
        if device:
            give = {k: dev(v) for k, v in give.items()}
            torch.cuda.synchronize()
        call(give)                                                          # (raises on any status but FOVPT_OK, a HIP error among them)
        for k in meshes:
            self.vtx[3 * k:3 * k + 3] = new[k]
        self.marked |= set(meshes)
        self.check()

    def check(self):
        r = self.r
        r.synchronize()
        p, n = debug_buffer(r, "scene_vertices")
        assert n == self.vtx.size * 4
        assert np.array_equal(bits(r.download(p, np.empty((NMESH * 3, 3), F))), bits(self.vtx))
        if self.tracking and self.marked:
            p, n = debug_buffer(r, "scene_vertices_prev")
            prev = r.download(p, np.empty((NMESH * 3, 3), F))
            rows = np.concatenate([np.arange(3 * k, 3 * k + 3) for k in sorted(self.marked)])
            assert np.array_equal(bits(prev[rows]), bits(self.vtx_step[rows]))
        r.launchParams.frame.subframe_index = 0
        r.render()                                                          # (waits for the refit; synchronous)
        assert r.downloadPixels().shape == (SIZE[1], SIZE[0])


@pytest.fixture(scope="module")
def scene():
    s = Scene()
    yield s
    s.r.close()


# ---- 1. every source over every list --------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", SOURCES)
def test_every_list_through_a_source(scene, source):
    assert [len(v) for v in LISTS.values()] == [1, BATCH, BATCH + 1, 2 * BATCH, NMESH, 33, 20]
    for name, meshes in LISTS.items():
        scene.update(source, meshes)


# ---- 2. the two batches of a morphed call ---------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
def test_morph_poses_with_palettes_on_an_irregular_subset(scene, form):
    """66 poses.  First: 32 of them carry a palette, none of the first five, and the last pose is the 32nd: the batch with
    palettes fills exactly with the list's last pose while the other, filled once at its 32nd pose, ends with 2.  Then the
    other way round: 34 with a palette, and the 32nd without one comes last."""
    rng = np.random.default_rng(5)
    middle = sorted(rng.choice(np.arange(5, NMESH - 1), BATCH - 1, replace=False).tolist())
    with_palette = middle + [NMESH - 1]
    assert len(with_palette) == BATCH and with_palette[0] >= 5 and np.any(np.diff(with_palette) > 1)
    without = [k for k in range(NMESH) if k not in with_palette]
    assert len(without) == NMESH - BATCH and without[-1] != NMESH - 1
    scene.update("morphed_" + form, list(range(NMESH)), with_palette)
    scene.update("morphed_" + form, list(range(NMESH)), [k for k in range(NMESH) if k not in middle + [NMESH - 1]])
    scene.update("morphed_" + form, list(range(NMESH)), [NMESH - 1])      # one pose with a palette, the last
    scene.update("morphed_" + form, list(range(NMESH)), list(range(1, NMESH)))      # one pose without, the first


# ---- 3. the copies of fovpt_temporal_motion's tracking --------------------------------------------------------------------
@pytest.mark.parametrize("source", ["vertices_host", "vertices_device", "transforms", "skinned_host", "morphed_skinned_device"])
def test_first_touched_meshes_of_an_interval(source):
    """With tracking on, an update copies the positions of the meshes it is the interval's first to touch.  Meshes 34 .. 65 (32:
    one full batch); then all 66 (34 first-touched -- a full batch and 2 -- of which the last listed mesh is none); then 10 that are
    all marked (nothing to launch); and after the interval's end a list of 33."""
    s = Scene(tracking=True)
    s.update("vertices_host", list(range(NMESH)))                          # positions that are not the rest positions
    s.step()
    s.update(source, list(range(NMESH - BATCH, NMESH)))
    assert len(s.marked) == BATCH
    s.update(source, list(range(NMESH)))
    s.update(source, list(range(20, 30)))
    s.step()
    s.update(source, LISTS["33"])
    s.r.close()
