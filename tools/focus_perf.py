"""fovpt_focus at BASELINE C3 (262,144-triangle atrium, 1920 x 1080, radii 148 / 482, spp 1 / 2 / 8): device time per call from
HIP events recorded on the library's stream around --calls calls back to back after a warm-up.  In one process, alternately,
--reps times each, all with a caller's G-buffer (fovpt_temporal_gbuffer's, of the fovpt_post step) but TRACE:
    COPY      FIXED, strength 0: every tile of k_focus_gather a copy (k_focus_radius and the gather's staging remain)
    DEFAULTS  fovpt_focus_defaults (AUTO, max_radius 6) with the gaze on the atrium's nearest column; strength 8 x that column's
              distance: the atrium is hundreds of units deep, the literal 8 per unit of 1 / distance blurs nothing there (RAW)
    WORST     FIXED, every pixel at max_radius 8: about 227 covering taps per pixel
    METER     the AUTO meter alone: AUTO minus FIXED at strength 0, for the defaults' disc (radius 12) and the largest (64)
    TRACE     DEFAULTS with the call's own G-buffer trace
    FIXED     fovpt_expose FIXED: the yardstick of a plain full-frame pass (reads 16 bytes, writes 20 per pixel)
    RENDER    one fovpt_render
from the accum buffer into the renderer's own buffers, and prints one JSON line: the median over the repetitions and the spread
(min, max) of each, and the shares of sharp and capped pixels of DEFAULTS.  Nothing here is a threshold.
Kernel statistics are a separate run:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/focus_perf.py --calls 20 --reps 1"""
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
    gb = r.downloadGBuffer()
    t = np.where(gb["prim"] != 0xffffffff, gb["position"][..., 3], np.inf)
    t[:64], t[-64:], t[:, :64], t[:, -64:] = np.inf, np.inf, np.inf, np.inf      # (the whole disc inside the frame)
    gy, gx = np.unravel_index(int(np.argmin(t)), t.shape)                        # the nearest surface: a column
    nearest = float(t[gy, gx])
    r.launchParams.frame.c.x, r.launchParams.frame.c.y = int(gx), int(gy)
    r.render()
    r.post()
    g = r.temporal_gbuffer()                                  # the rendered frame's

    def fc(**d):
        c = r.focus_defaults()
        for k, v in d.items():
            setattr(c, k, v)
        return c

    defaults = fc(strength=r.focus_defaults().strength * nearest)                # 8 pixels per unit of |focus / t - 1|
    fixed0, auto0, auto0_64 = fc(mode=abi.FOCUS_FIXED, strength=0.0), fc(strength=0.0), fc(strength=0.0, meter_radius=64)
    worst = fc(mode=abi.FOCUS_FIXED, max_radius=8, strength=1e6, focus_distance=1e-3)
    expose_fixed = r.expose_defaults()
    expose_fixed.mode = abi.EXPOSE_FIXED
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

    cases = dict(COPY=lambda: r.focus(fixed0, g), DEFAULTS=lambda: r.focus(defaults, g), RAW=lambda: r.focus(fc(), g), WORST=lambda: r.focus(worst, g),
                 AUTO0=lambda: r.focus(auto0, g), AUTO0_64=lambda: r.focus(auto0_64, g), TRACE=lambda: r.focus(defaults),
                 FIXED=lambda: r.expose(expose_fixed), RENDER=lambda: r.render_async())
    ms = {k: [] for k in cases}
    for _ in range(reps):                                     # alternately
        for k, fn in cases.items():
            ms[k].append(per_call(fn))
    out = dict(config="C3", size=list(size), calls=calls, reps=reps, device=torch.cuda.get_device_name(0), gaze=[int(gx), int(gy)], nearest=round(nearest, 2))
    for k, v in ms.items():
        out["ms_" + k] = round(float(np.median(v)), 4)
        out["spread_" + k] = [round(min(v), 4), round(max(v), 4)]
    out["ms_METER_12"] = round(out["ms_AUTO0"] - out["ms_COPY"], 4)
    out["ms_METER_64"] = round(out["ms_AUTO0_64"] - out["ms_COPY"], 4)
    out["COPY_over_FIXED"] = round(out["ms_COPY"] / out["ms_FIXED"], 2)
    out["RENDER_over_WORST"] = round(out["ms_RENDER"] / out["ms_WORST"], 2)
    n = size[0] * size[1]
    coc = torch.zeros((size[1], size[0]), dtype=torch.float32, device="cuda")
    for name, c in (("DEFAULTS", defaults), ("WORST", worst)):
        r.focus_reset()
        r.focus(c, g, None, None, None, coc.data_ptr())
        r.synchronize()
        rad = coc.cpu().numpy()
        out["radii_" + name] = dict(below_half=round(float((rad < 0.5).sum()) / n, 4), capped=round(float((rad == c.max_radius).sum()) / n, 4),
                                    mean=round(float(rad.mean()), 3))
        if name == "DEFAULTS":
            s = r.focus_state()
            out["state"] = dict(focus=round(float(s.focus), 2), count=int(s.count))
    print(json.dumps(out), flush=True)
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    main(args.calls, args.warmup, args.reps)
