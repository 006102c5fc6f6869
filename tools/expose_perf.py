"""fovpt_expose at BASELINE C3 (262,144-triangle atrium, 1920 x 1080, radii 148 / 482, spp 1 / 2 / 8): device time per call from
HIP events recorded on the library's stream around --calls calls back to back after a warm-up.  In one process, alternately,
--reps times each:
    GAZE    fovpt_expose AUTO, METER_GAZE (the defaults): k_expose_meter<gaze>, k_expose_adapt, k_expose_apply
    FRAME   fovpt_expose AUTO, METER_FRAME
    FIXED   fovpt_expose FIXED: k_expose_apply alone
    DN0     fovpt_denoise with all iteration counts 0: reads accum, writes colour + rgba8 once (FIXED's traffic)
all from the accum buffer into the renderer's own buffers, and prints one JSON line: the median over the repetitions and the
spread (min, max) of each.  Expectations to examine, not thresholds: FIXED is about DN0; AUTO is about
one more read of the frame (33 MB) plus two small launches.  Kernel statistics are a separate run:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/expose_perf.py --calls 20 --reps 1"""
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
    gaze, frame, fixed = r.expose_defaults(), r.expose_defaults(), r.expose_defaults()
    frame.metering = abi.METER_FRAME
    fixed.mode = abi.EXPOSE_FIXED
    dn0 = r.denoise_defaults()
    dn0.iterations_fovea = dn0.iterations_middle = dn0.iterations_periphery = dn0.iterations_uniform = 0
    cases = dict(GAZE=lambda: r.expose(gaze), FRAME=lambda: r.expose(frame), FIXED=lambda: r.expose(fixed), DN0=lambda: r.denoise(dn0))
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
    out["FIXED_over_DN0"] = round(med["FIXED"] / med["DN0"], 3)
    out["GAZE_over_FIXED"] = round(med["GAZE"] / med["FIXED"], 3)
    out["FRAME_over_FIXED"] = round(med["FRAME"] / med["FIXED"], 3)
    s = r.expose_state()
    out["state"] = dict(ev=round(s.ev, 4), exposure=round(s.exposure, 5), weight_total=int(s.weight_total), steps=int(s.steps))
    print(json.dumps(out), flush=True)
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    main(args.calls, args.warmup, args.reps)
