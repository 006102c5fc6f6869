"""Seed -> parameters of one post-processing fuzz case (tests/test_postprocess_fuzz_gpu.py).  Pure numpy, no GPU: the CPU
suite (tests/test_postprocess_fuzz_cpu.py) runs this generator alone and checks that the default seed range reaches every
edge listed below, so that an edit here cannot quietly drop one."""
import math
import os

import numpy as np

from fovpathtracing_optixcodelatest_amd import abi

DEFAULT_SEEDS = range(0, 48)
SEEDS = range(int(os.environ.get("FOVPT_FUZZP_FROM", DEFAULT_SEEDS.start)), int(os.environ.get("FOVPT_FUZZP_TO", DEFAULT_SEEDS.stop)))  # widen for a sweep
# the first seeds' frame sizes: narrower / shorter than one 4 x 4 block (the P pass has a zero grid), widths one short of and
# one over a multiple of 64 (the denoiser's 64 x 4 tiles) with heights not a multiple of 4, and 2 x 50 (no P pass at all)
EDGE_SHAPES = [(1, 1), (1, 37), (37, 1), (3, 3), (4, 4), (5, 9), (63, 3), (65, 5), (129, 7), (2, 50)]
SCENES = ("atrium", "box", "soup")
RADII = ("zero", "equal", "ordinary", "beyond")
DENOISE_SIGMAS = {"color_sigma": 8.0, "normal_sigma": 0.5, "albedo_sigma": 0.2}           # (the defaults)
RECONSTRUCT_SIGMAS = {"normal_sigma": 0.5, "depth_sigma": 0.05}
LEVELS = ("iterations_fovea", "iterations_middle", "iterations_periphery", "iterations_uniform")


def _sigma(rng, default):
    """An endpoint of [SIGMA_MIN, SIGMA_MAX] (30 %), log-uniform over all of it (35 %), or log-uniform within a factor of 10
    of the default, where the edge stopping does neither nothing nor everything (35 %)."""
    u = rng.random()
    if u < 0.15:
        return abi.SIGMA_MIN
    if u < 0.3:
        return abi.SIGMA_MAX
    lo, hi = (math.log(abi.SIGMA_MIN), math.log(abi.SIGMA_MAX)) if u < 0.65 else (math.log(default / 10), math.log(default * 10))
    return float(np.float32(math.exp(rng.uniform(lo, hi))))


def params(seed):
    rng = np.random.default_rng(31000 + seed)
    if seed < len(EDGE_SHAPES):
        w, h = EDGE_SHAPES[seed]
    else:
        w, h = int(rng.integers(1, 201)), int(rng.integers(1, 131))
    p = dict(seed=seed, size=(w, h), scene=SCENES[seed % 3], scene_seed=int(rng.integers(1, 1000)))
    # the gaze anywhere around the frame: M and F offsets (gaze - radius) wrap as uint32
    p["gaze"] = (int(rng.integers(-40, w + 41)), int(rng.integers(-40, h + 41)))
    kind = RADII[(seed // 3) % 4] if seed < 24 else RADII[int(rng.integers(0, 4))]
    diag = int(math.ceil(math.hypot(w, h)))
    if kind == "zero":
        radii = (0, 0)
    elif kind == "equal":
        r = int(rng.integers(0, 60))
        radii = (r, r)
    elif kind == "ordinary":
        r = int(rng.integers(0, 40))
        radii = (r, r + int(rng.integers(1, 80)))
    else:
        r_out = diag + int(rng.integers(1, 100))
        radii = (min(int(rng.integers(0, diag + 20)), r_out), r_out)
    p["radii_kind"], p["radii"] = kind, radii
    p["uniform"] = int(rng.random() < 0.25)
    p["accumulate"] = int(rng.random() < 0.3)
    p["spp"] = tuple(int(x) for x in rng.integers(1, 5, 4))                 # periphery, middle, fovea, uniform
    p["max_depth"] = int(rng.integers(1, 5))
    # remodulate 0 on a context without guides: no denoise (it needs them), reconstruct without the albedo guide
    p["write_guides"] = 0 if rng.random() < 0.12 else 1
    # denoise: every iteration count 0 .. 5 (all zeros and all fives on fixed seeds)
    if seed % 12 == 5:
        its = [0, 0, 0, 0]
    elif seed % 12 == 11:
        its = [abi.DENOISE_MAX_ITERATIONS] * 4
    else:
        its = [int(x) for x in rng.integers(0, abi.DENOISE_MAX_ITERATIONS + 1, 4)]
    p["denoise"] = dict(zip(LEVELS, its), **{k: _sigma(rng, v) for k, v in DENOISE_SIGMAS.items()}) if p["write_guides"] else None
    # reconstruct
    u = rng.random()
    support = 1.0 if u < 0.3 else 2.0 if u < 0.6 else float(np.float32(rng.uniform(1.0, 2.0)))
    rc = dict(support=support, levels=int(rng.integers(0, 4)), remodulate=int(rng.random() < 0.7) if p["write_guides"] else 0,
              **{k: _sigma(rng, v) for k, v in RECONSTRUCT_SIGMAS.items()})
    p["reconstruct"] = rc
    p["reconstruct_input"] = "denoised" if p["denoise"] is not None and rng.random() < 0.4 else "accum"
    p["caller_buffers"] = bool(rng.random() < 0.35)
    return p
