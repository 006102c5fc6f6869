"""fovpt_bloom at BASELINE C3 (262,144-triangle atrium, 1920 x 1080, radii 148 / 482, spp 1 / 2 / 8): device time per call from HIP
events recorded on the library's stream around --calls calls back to back after a warm-up.  In one process, alternately, --reps
times each:
    BLOOM    fovpt_bloom with the defaults (KARIS, 6 levels): k_bloom_prefilter, the levels down and up, k_bloom_composite
    GAINS    the defaults with FOVPT_BLOOM_GAINS: four writer searches per texel of the first level
    L8       the defaults with 8 levels
    STATE    the defaults with FOVPT_BLOOM_EXPOSURE_STATE behind one AUTO fovpt_expose: the exposure from the device record
    FIXED    fovpt_expose FIXED: the plain full-frame pass (reads the frame, writes colour + rgba8 once)
    RENDER   one fovpt_render
all from the accum buffer into the renderer's own buffers, and prints one JSON line: the median over the repetitions and the
spread (min, max) of each.  Numbers to report, not thresholds.  Kernel statistics are a separate run:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bloom_perf.py --calls 20 --reps 1"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fovpathtracing_optixcodelatest_amd import abi, renderer, scenes  # noqa: E402


def main(calls, warmup, reps):
    size = (1920, 1080)
    cfg = abi.Config.reference_default()
    cfg.r_inner, cfg.r_outer = 148, 482
    cfg.spp_periphery, cfg.spp_middle, cfg.spp_fovea = 1, 2, 8
    cfg.write_guides = 1
    r = renderer.SampleRenderer(scenes.atrium(262144))
    r.resize(size)
    cam = scenes.ATRIUM_CAMERA
    r.setCamera(renderer.Camera(cam["eye"], cam["lookat"], cam["up"], cam["fovy"], size[0] / size[1]))
    r.setProbe(renderer.ProbeData(scenes.ambient_probe(size[0], size[1], 2.5)).BuildCDF())
    r.config = cfg
    r.launchParams.frame.c.x, r.launchParams.frame.c.y = size[0] // 2, size[1] // 2
    r.render()
    base, gains, l8, state = (r.bloom_defaults() for _ in range(4))
    gains.flags |= abi.BLOOM_GAINS
    l8.levels = 8
    state.flags |= abi.BLOOM_EXPOSURE_STATE
    fixed = r.expose_defaults()
    fixed.mode = abi.EXPOSE_FIXED
    r.expose(r.expose_defaults())                             # one AUTO step: STATE finds a record with steps != 0

    cases = dict(BLOOM=lambda: r.bloom(base), GAINS=lambda: r.bloom(gains), L8=lambda: r.bloom(l8), STATE=lambda: r.bloom(state),
                 FIXED=lambda: r.expose(fixed), RENDER=lambda: r.render_async())
    st = torch.cuda.ExternalStream(r.stream)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def per_call(fn):
        for _ in range(warmup):
            fn()
        r.synchronize()
        a.record(st)
        for _ in range(calls):
            fn()
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b) / calls

    ms = {k: [] for k in cases}
    for _ in range(reps):                                     # alternately
        for k, fn in cases.items():
            ms[k].append(per_call(fn))
    out = dict(config="C3", size=list(size), calls=calls, reps=reps, device=torch.cuda.get_device_name(0))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    for k, v in ms.items():
        out["ms_" + k] = round(med[k], 4)
        out["spread_" + k] = [round(min(v), 4), round(max(v), 4)]
    for k in ("BLOOM", "GAINS", "L8"):
        out[k + "_over_FIXED"] = round(med[k] / med["FIXED"], 3)
    print(json.dumps(out), flush=True)
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    main(args.calls, args.warmup, args.reps)
