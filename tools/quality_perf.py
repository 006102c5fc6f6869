"""fovpt_quality at BASELINE C3 (262,144-triangle atrium, 1920 x 1080, radii 148 / 482, spp 1 / 2 / 8): device time per call from HIP
events recorded on the library's stream around --calls calls back to back after a warm-up.  In one process, alternately, --reps
times each; the measurements compare the frame buffer with the rgba8 image fovpt_expose FIXED made of the same frame, into a device
record of the caller's:
    NONE / SSIM / PROFILE / BOTH      fovpt_quality with no flags, with FOVPT_QUALITY_SSIM, with FOVPT_QUALITY_PROFILE, with both
    BOTH_CLASS                        both flags and the class map written
    AUTO_GAZE                         fovpt_expose AUTO, METER_GAZE: one writer search per pixel and a two-kernel reduction, the nearest
                                      existing stage
    FIXED                             fovpt_expose FIXED: the yardstick of a plain full-frame pass
    RENDER                            one fovpt_render
and prints one JSON line: the median over the repetitions and the spread (min, max) of each, and each fovpt_quality variant's ratio
to AUTO_GAZE of the same run.  Nothing here is a threshold.  Kernel statistics are a separate run:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/quality_perf.py --calls 20 --reps 1"""
import argparse
import ctypes as C
import json
import math
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
    r = renderer.SampleRenderer(scenes.atrium(262144))
    r.resize(size)
    cam = scenes.ATRIUM_CAMERA
    r.setCamera(renderer.Camera(cam["eye"], cam["lookat"], cam["up"], cam["fovy"], size[0] / size[1]))
    r.setProbe(renderer.ProbeData(scenes.ambient_probe(size[0], size[1], 2.5)).BuildCDF())
    r.config = cfg
    r.launchParams.frame.c.x, r.launchParams.frame.c.y = size[0] // 2, size[1] // 2
    r.render()
    expose_fixed = r.expose_defaults()
    expose_fixed.mode = abi.EXPOSE_FIXED
    expose_fixed.exposure = 12.0                              # (not the resolve's 16: the two images differ)
    expose_auto = r.expose_defaults()
    r.expose(expose_fixed)
    ref = r.expose_buffers()[1]
    sums = torch.zeros(C.sizeof(abi.QualitySums), dtype=torch.uint8, device="cuda")
    classes = torch.zeros(size[0] * size[1], dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def qc(flags):
        c = r.quality_defaults()
        c.flags = flags
        return c

    variants = dict(NONE=(qc(0), None), SSIM=(qc(abi.QUALITY_SSIM), None), PROFILE=(qc(abi.QUALITY_PROFILE), None),
                    BOTH=(qc(abi.QUALITY_SSIM | abi.QUALITY_PROFILE), None), BOTH_CLASS=(qc(abi.QUALITY_SSIM | abi.QUALITY_PROFILE), classes.data_ptr()))
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

    cases = {k: (lambda c=c, p=p: r.qualityAsync(ref, None, c, sums.data_ptr(), p)) for k, (c, p) in variants.items()}
    cases["AUTO_GAZE"] = lambda: r.expose(expose_auto)
    cases["FIXED"] = lambda: r.expose(expose_fixed)
    cases["RENDER"] = lambda: r.render_async()
    ms = {k: [] for k in cases}
    for _ in range(reps):                                     # alternately
        for k, fn in cases.items():
            ms[k].append(per_call(fn))
    out = dict(config="C3", size=list(size), calls=calls, reps=reps, device=torch.cuda.get_device_name(0))
    for k, v in ms.items():
        out["ms_" + k] = round(float(np.median(v)), 4)
        out["spread_" + k] = [round(min(v), 4), round(max(v), 4)]
    for k in variants:
        out[k + "_over_AUTO_GAZE"] = round(out["ms_" + k] / out["ms_AUTO_GAZE"], 2)
    r.expose(expose_fixed)                                    # (AUTO wrote the exposed buffers last)
    r.qualityAsync(ref, None, variants["BOTH"][0], sums.data_ptr())
    r.synchronize()
    s = abi.QualitySums.from_buffer_copy(sums.cpu().numpy().tobytes())
    sc = r.quality_scores(s)
    out["psnr"] = {k: round(v, 2) for k, v in sc["psnr"].items() if math.isfinite(v)}      # (no NaN or Infinity in the JSON line)
    out["ssim"] = {k: round(v, 4) for k, v in sc["ssim"].items() if math.isfinite(v)}
    print(json.dumps(out), flush=True)
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    main(args.calls, args.warmup, args.reps)
