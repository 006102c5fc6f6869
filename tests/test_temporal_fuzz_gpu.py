"""A seeded fuzz of fovpt_temporal on the GPU: random scenes (the atrium, the slab and box, the triangle soup of
test_postprocess_fuzz_gpu.py), frame sizes (odd ones and ones below one 4 x 4 block included), camera paths, gazes off the
frame, radii, FOV_OFF and config values at the ends of their ranges, every step bit for bit against tests/temporal_ref.py on
the GPU's own inputs.  FOVPT_FUZZT_FROM / FOVPT_FUZZT_TO widen the sweep."""
import math
import os

import numpy as np
import pytest

from fovpathtracing_optixcodelatest_amd import abi, renderer, scenes

from common import cfg_foveated, cfg_uniform, make_gpu
from gpu_common import BOX_CAMERA, box_model
from temporal_common import Checker
from test_postprocess_fuzz_gpu import SOUP_CAMERA, _soup

pytestmark = pytest.mark.gpu
DEFAULT_SEEDS = range(0, 24)
SEEDS = range(int(os.environ.get("FOVPT_FUZZT_FROM", DEFAULT_SEEDS.start)), int(os.environ.get("FOVPT_FUZZT_TO", DEFAULT_SEEDS.stop)))
EDGE_SHAPES = [(1, 1), (3, 5), (4, 4), (65, 5), (2, 50), (129, 7)]
M = abi.TEMPORAL_MAX_HISTORY


def params(seed):
    rng = np.random.default_rng(47000 + seed)
    w, h = EDGE_SHAPES[seed] if seed < len(EDGE_SHAPES) else (int(rng.integers(1, 201)), int(rng.integers(1, 131)))
    p = dict(size=(w, h), scene=("atrium", "box", "soup")[seed % 3], scene_seed=int(rng.integers(1, 1000)))
    p["gaze"] = [(int(rng.integers(-40, w + 41)), int(rng.integers(-40, h + 41))) for _ in range(4)]
    r_in = int(rng.integers(0, 40))
    p["radii"] = (r_in, r_in + int(rng.integers(0, 80)))
    p["uniform"] = int(rng.random() < 0.25)
    p["spp"] = tuple(int(x) for x in rng.integers(1, 4, 4))
    pick = lambda lo, hi, f: lo if (u := rng.random()) < 0.2 else hi if u < 0.4 else f(lo, hi)
    caps = ("history_fovea", "history_middle", "history_periphery", "history_uniform")
    d = {k: pick(1, M, lambda a, b: int(rng.integers(a, b + 1))) for k in caps}
    d["normal_tolerance"] = pick(0.0, 4.0, lambda a, b: float(np.float32(rng.uniform(a, b))))
    d["depth_tolerance"] = pick(0.0, 1.0, lambda a, b: float(np.float32(rng.uniform(a, b))))
    p["temporal"] = d
    p["motion"] = [tuple(float(x) for x in rng.normal(0, 1, 6)) for _ in range(4)]    # eye and look-at steps, scene units / 10
    p["frames"] = int(rng.integers(2, 5))
    return p


def _scene(p):
    if p["scene"] == "atrium":
        tris = int(np.random.default_rng(p["scene_seed"]).integers(1000, 6000))
        return scenes.atrium(tris, seed=p["scene_seed"]), scenes.ATRIUM_CAMERA, scenes.ambient_probe(96, 54, 2.5), 100.0
    if p["scene"] == "box":
        return box_model(), BOX_CAMERA, scenes.sky_probe(), 0.3
    return _soup(p["scene_seed"]), SOUP_CAMERA, scenes.ambient_probe(32, 16, 1.0), 0.5


@pytest.mark.parametrize("seed", SEEDS)
def test_random_temporal(oracle, seed):
    p = params(seed)
    model, cam, probe, scale = _scene(p)
    if p["uniform"]:
        cfg = cfg_uniform(p["spp"][3])
    else:
        cfg = cfg_foveated(p["radii"][0], p["radii"][1], p["spp"][:3])
    r = make_gpu(model, probe, cam, p["size"], cfg, gaze=p["gaze"][0])
    ck = Checker(oracle, r, p["temporal"])
    eye, look = np.array(cam["eye"], np.float64), np.array(cam["lookat"], np.float64)
    w, h = p["size"]
    for k in range(p["frames"]):
        mv = np.array(p["motion"][k]) * scale
        eye, look = eye + mv[:3], look + mv[3:]
        r.setCamera(renderer.Camera(tuple(eye), tuple(look), cam["up"], cam["fovy"], w / float(h)))
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = (v & 0xffffffff for v in p["gaze"][k])
        r.render()
        ck.step()
    r.close()


def test_the_seeds_reach_the_edges():
    ps = [params(s) for s in DEFAULT_SEEDS]
    for k in ("history_fovea", "history_middle", "history_periphery", "history_uniform"):
        vals = {q["temporal"][k] for q in ps}
        assert 1 in vals and M in vals, k
    for k, hi in (("normal_tolerance", 4.0), ("depth_tolerance", 1.0)):
        vals = {q["temporal"][k] for q in ps}
        assert 0.0 in vals and hi in vals, k
    assert any(q["uniform"] for q in ps) and not all(q["uniform"] for q in ps)
    assert any(q["size"][0] % 2 and q["size"][1] % 2 for q in ps)
    assert any(min(q["size"]) < 4 for q in ps)
    assert {q["scene"] for q in ps} == {"atrium", "box", "soup"}
    assert any(not (0 <= g[0] < q["size"][0]) for q in ps for g in q["gaze"])
