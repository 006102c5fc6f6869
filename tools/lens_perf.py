"""fovpt_lens at BASELINE C3 (262,144-triangle atrium, 1920 x 1080, radii 148 / 482, spp 1 / 2 / 8): device time per call from HIP
events recorded on the library's stream around --calls calls back to back after a warm-up.  In one process, alternately, --reps
times each, all reading the colour fovpt_expose FIXED left in the renderer's own buffers, with fovpt_lens_defaults fitted to the
frame (lens_for_frame):
    NEAREST / BILINEAR / BICUBIC      the filter, with the defaults' distinct chroma factors: three lookups per pixel
    *_EQUAL                           the same with the three chroma factors equal: one lookup of 16-byte taps
    BILINEAR_TO                       BILINEAR (distinct) re-aimed at the camera turned by 2 degrees
    FIXED                             fovpt_expose FIXED: the yardstick of a plain full-frame pass (reads 16 bytes, writes 20 per pixel)
    RENDER                            one fovpt_render
and prints one JSON line: the median over the repetitions and the spread (min, max) of each, each variant's ratio to FIXED, and its
share of border pixels (all three channels the border's: measured on a constant image).  Nothing here is a threshold (DESIGN.md,
section 25).  Kernel statistics are a separate run:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/lens_perf.py --calls 20 --reps 1"""
import argparse
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
    r.expose(expose_fixed)
    exposed = r.expose_buffers()[0]

    # the camera turned by 2 degrees about its up axis
    e, l = np.array(cam["eye"], np.float64), np.array(cam["lookat"], np.float64)
    a2, v = math.radians(2.0), l - e
    v = np.array([math.cos(a2) * v[0] + math.sin(a2) * v[2], v[1], -math.sin(a2) * v[0] + math.cos(a2) * v[2]])
    to = renderer.Camera(tuple(e), tuple(e + v), cam["up"], cam["fovy"], size[0] / size[1])

    def lc(flt, equal):
        c = r.lens_for_frame(r.lens_defaults(), *size)
        c.filter = flt
        if equal:
            c.chroma = (1.0, 1.0, 1.0)
        return c

    names = {abi.LENS_NEAREST: "NEAREST", abi.LENS_BILINEAR: "BILINEAR", abi.LENS_BICUBIC: "BICUBIC"}
    variants = {}
    for flt, name in names.items():
        variants[name] = (lc(flt, False), None)
        variants[name + "_EQUAL"] = (lc(flt, True), None)
    variants["BILINEAR_TO"] = (lc(abi.LENS_BILINEAR, False), to)
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

    cases = {k: (lambda c=c, t=t: r.lens(c, t, exposed)) for k, (c, t) in variants.items()}
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
    ones = torch.ones((size[1], size[0], 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for k, (c, t) in variants.items():
        out[k + "_over_FIXED"] = round(out["ms_" + k] / out["ms_FIXED"], 2)
        r.lens(c, t, ones.data_ptr())
        col, _ = r.downloadLens()
        out["border_" + k] = round(float((col[..., :3] == 0).all(axis=-1).mean()), 4)
    print(json.dumps(out), flush=True)
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    main(args.calls, args.warmup, args.reps)
