"""A seeded fuzz of fovpt_post against the separate stage calls on a twin context: frame sizes, gazes off the frame, radii,
FOV_OFF, accumulation, scenes and stage configs drawn by tests/postprocess_fuzz.py, a random valid stage mask and random
history caps and tolerances on top, three frames with the camera and gaze moving, every output and the history bit for bit."""
import os

import numpy as np
import pytest

import post_ref as po
import postprocess_fuzz as pf
from fovpathtracing_optixcodelatest_amd import abi, renderer

from common import make_gpu
from post_common import D, M, R, T, pcfg, same, separate
from test_postprocess_fuzz_gpu import _config, _scene

pytestmark = pytest.mark.gpu
# postprocess_fuzz's seeds 6 .. 11: frames one short of and one over a multiple of the 64-pixel tile with heights no multiple of
# 4, a frame without a periphery pass, and two random sizes; FOVPT_FUZZP_FROM / FOVPT_FUZZP_TO widen the sweep (0 .. 5 are the
# frames narrower than one block)
DEFAULT_SEEDS = range(6, 12)
SEEDS = range(int(os.environ.get("FOVPT_FUZZP_FROM", DEFAULT_SEEDS.start)), int(os.environ.get("FOVPT_FUZZP_TO", DEFAULT_SEEDS.stop)))
FRAMES = 3


def chain(seed):
    """-> (params of postprocess_fuzz, stage mask, temporal config dict)"""
    p = pf.params(seed)
    rng = np.random.default_rng(77000 + seed)
    masks = [s for s in po.VALID_STAGES if p["denoise"] is not None or not s & D]
    if rng.random() < 0.5:                                  # every other case one of the masks that run the fused kernel
        masks = [s for s in masks if s & R and s & T]
    stages = masks[int(rng.integers(0, len(masks)))]
    Mh = abi.TEMPORAL_MAX_HISTORY
    caps = [int(rng.choice([1, 2, 3, 8, Mh])) for _ in range(4)]
    t = dict(zip(("history_fovea", "history_middle", "history_periphery", "history_uniform"), caps),
             normal_tolerance=float(np.float32(rng.choice([0.0, 0.1, 0.5, 4.0]))), depth_tolerance=float(np.float32(rng.choice([0.0, 0.02, 0.2, 1.0]))))
    return p, stages, t


def test_the_seeds_reach_the_stage_masks():
    seen = {chain(s)[1] for s in DEFAULT_SEEDS}
    assert any(s & R and s & T for s in seen) and len(seen) >= 3, seen     # the fused kernel, and other compositions


@pytest.mark.parametrize("seed", SEEDS)
def test_random_post(seed):
    p, stages, t = chain(seed)
    model, cam, probe = _scene(p)
    (w, h), gaze = p["size"], p["gaze"]
    a, b = (make_gpu(model, probe, cam, (w, h), _config(p), gaze=gaze) for _ in range(2))
    pc = pcfg(stages, p["denoise"], p["reconstruct"], t)
    for k in range(FRAMES):
        for r in (a, b):
            eye = tuple(np.float32(cam["eye"]) * np.float32(1.0 + 0.04 * k) + np.float32([0.3 * k, 0.1 * k, 0.0]))
            r.setCamera(renderer.Camera(eye, cam["lookat"], cam["up"], cam["fovy"], w / float(h)))
            r.launchParams.frame.c.x, r.launchParams.frame.c.y = (gaze[0] + 5 * k) & 0xffffffff, (gaze[1] - 3 * k) & 0xffffffff
            r.render()
        separate(a, pc, out_motion=a.motion_buffer() if stages & M else None)
        b.post(pc, out_motion=b.motion_buffer() if stages & M else None)
        same(a, b, stages, (p, stages, t, k))
    a.close()
    b.close()
