"""A seeded fuzz of fovpt_temporal_motion on the GPU: random subsets of the atrium's meshes jittered or turned through random
update flags (refit or rebuild, host arrays or device pointers, sometimes twice between steps), random caps and tolerances, a
random gaze and camera path, sizes around 97 x 61, an occasional step through fovpt_temporal, motion vectors on and off: every
step bit for bit against tests/temporal_motion_ref.py on the GPU's own inputs.  FOVPT_FUZZTM_FROM / FOVPT_FUZZTM_TO widen the
sweep."""
import os

import numpy as np
import pytest

from fovpathtracing_optixcodelatest_amd import abi, renderer, scenes

from common import cfg_foveated, cfg_uniform, make_gpu
from temporal_motion_common import MotionChecker
from test_refit_gpu import jitter, rotate_translate

pytestmark = pytest.mark.gpu
DEFAULT_SEEDS = range(0, 8)
SEEDS = range(int(os.environ.get("FOVPT_FUZZTM_FROM", DEFAULT_SEEDS.start)), int(os.environ.get("FOVPT_FUZZTM_TO", DEFAULT_SEEDS.stop)))
M = abi.TEMPORAL_MAX_HISTORY
FRAMES = 5
CAM = scenes.ATRIUM_CAMERA


def params(seed):
    rng = np.random.default_rng(91000 + seed)
    w, h = 97 + int(rng.integers(-12, 13)), 61 + int(rng.integers(-8, 9))
    p = dict(size=(w, h), scene_seed=int(rng.integers(1, 1000)))
    p["gaze"] = [(int(rng.integers(-20, w + 21)), int(rng.integers(-20, h + 21))) for _ in range(FRAMES)]
    r_in = int(rng.integers(0, 30))
    p["radii"] = (r_in, r_in + int(rng.integers(0, 50)))
    p["uniform"] = int(rng.random() < 0.25)
    pick = lambda lo, hi, f: lo if (u := rng.random()) < 0.15 else hi if u < 0.3 else f(lo, hi)
    d = {k: pick(1, M, lambda a, b: int(rng.integers(2, 9))) for k in ("history_fovea", "history_middle", "history_periphery", "history_uniform")}
    d["normal_tolerance"] = pick(0.0, 4.0, lambda a, b: float(np.float32(rng.uniform(0.05, 0.5))))
    d["depth_tolerance"] = pick(0.0, 1.0, lambda a, b: float(np.float32(rng.uniform(0.01, 0.1))))
    p["temporal"] = d
    p["camera"] = [tuple(float(x) for x in rng.normal(0, 8, 6)) for _ in range(FRAMES)]
    # per frame: up to two updates (share of the meshes, kind, amount seed, rebuild, device), then the kind of step
    p["updates"] = [[(float(rng.uniform(0.1, 1.0)), ("jitter", "turn")[int(rng.integers(0, 2))], int(rng.integers(0, 1 << 30)),
                      bool(rng.random() < 0.3), bool(rng.random() < 0.5)) for _ in range(int(rng.integers(0, 3)))] for _ in range(FRAMES)]
    p["plain"] = [bool(rng.random() < 0.2) for _ in range(FRAMES)]
    p["with_motion"] = [bool(rng.random() < 0.6) for _ in range(FRAMES)]
    return p


@pytest.mark.parametrize("seed", SEEDS)
def test_random_temporal_motion(oracle, seed):
    p = params(seed)
    model = scenes.atrium(2000, seed=p["scene_seed"])
    cfg = cfg_uniform(1) if p["uniform"] else cfg_foveated(p["radii"][0], p["radii"][1], (1, 1, 2))
    r = make_gpu(model, scenes.ambient_probe(48, 27, 2.5), CAM, p["size"], cfg, gaze=p["gaze"][0])
    ck = MotionChecker(oracle, r, p["temporal"])
    eye, look = np.array(CAM["eye"], np.float64), np.array(CAM["lookat"], np.float64)
    w, h = p["size"]
    nm = len(model.meshes)
    for k in range(FRAMES):
        for share, kind, s, rebuild, device in p["updates"][k]:
            rng = np.random.default_rng(s)
            ups = {}
            for m in np.flatnonzero(rng.random(nm) < share):
                v = ck.vtx[ck.first[m]:ck.first[m + 1]]
                if kind == "jitter":
                    ups[int(m)] = jitter(v, s + int(m), 15.0)
                else:
                    ups[int(m)] = rotate_translate(v, float(rng.uniform(-30, 30)), v.mean(axis=0), rng.normal(0, 20, 3))
            if ups or rebuild:
                ck.update(ups, rebuild=rebuild, device=device and bool(ups))
        mv = np.array(p["camera"][k])
        eye, look = eye + mv[:3], look + mv[3:]
        r.setCamera(renderer.Camera(tuple(eye), tuple(look), CAM["up"], CAM["fovy"], w / float(h)))
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = (v & 0xffffffff for v in p["gaze"][k])
        r.render()
        ck.step(plain=p["plain"][k], with_motion=p["with_motion"][k])
    r.close()


def test_the_seeds_reach_the_paths():
    ps = [params(s) for s in DEFAULT_SEEDS]
    ups = [u for q in ps for f in q["updates"] for u in f]
    assert {u[1] for u in ups} == {"jitter", "turn"}
    assert {(u[3], u[4]) for u in ups} == {(False, False), (False, True), (True, False), (True, True)}
    assert any(len(f) == 2 for q in ps for f in q["updates"]) and any(len(f) == 0 for q in ps for f in q["updates"])
    assert any(any(q["plain"]) for q in ps) and any(not x for q in ps for x in q["with_motion"]) and any(x for q in ps for x in q["with_motion"])
    assert any(q["uniform"] for q in ps) and not all(q["uniform"] for q in ps)
    assert any(q["size"][0] % 2 and q["size"][1] % 2 for q in ps)
