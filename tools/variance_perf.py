"""fovpt_variance and fovpt_variance_filter at BASELINE C3 (262,144-triangle atrium, 1920 x 1080, radii 148 / 482, spp 1 / 2 / 8): device
time per call from HIP events recorded on the library's stream around --calls calls back to back after a warm-up.  In one process,
alternately, --reps times each, all on the G-buffer and motion vectors one fovpt_post left (so no call here traces):
    VARIANCE_FIRST      fovpt_variance as a first step (a reset ahead of every call): the 7 x 7 spatial estimate runs everywhere
    VARIANCE_STEADY     fovpt_variance in steady state (the history at its cap): it runs nowhere
    VFILTER             fovpt_variance_filter at its defaults, filtering fovpt_post's colour
    DENOISE             fovpt_denoise at its defaults: the yardstick of the same kernel family
    FIXED               fovpt_expose FIXED: a plain full-frame pass
    RENDER              one fovpt_render
and prints one JSON line: the median over the repetitions and the spread (min, max) of each, and each new call's ratio to DENOISE.
--quality: on the 384 x 216 atrium path of tools/temporal_perf.py --sweep (tests/temporal_common.py), RMSE per foveation level of the
last frame against a 256-spp render of the same camera, for fovpt_post at its defaults alone, followed by the new filter with
luminance_sigma 1 / 2 / 4 / 8, and for fovpt_post with DENOISE; one JSON line.  Nothing here is a threshold.
Kernel statistics are a separate run:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/variance_perf.py --calls 20 --reps 1"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fovpathtracing_optixcodelatest_amd import abi, renderer, scenes  # noqa: E402


def perf(calls, warmup, reps):
    size = (1920, 1080)
    cfg = abi.Config.reference_default()
    cfg.r_inner, cfg.r_outer = 148, 482
    cfg.spp_periphery, cfg.spp_middle, cfg.spp_fovea = 1, 2, 8
    cfg.write_guides = 1                                      # (fovpt_denoise reads the guides)
    r = renderer.SampleRenderer(scenes.atrium(262144))
    r.resize(size)
    cam = scenes.ATRIUM_CAMERA
    r.setCamera(renderer.Camera(cam["eye"], cam["lookat"], cam["up"], cam["fovy"], size[0] / size[1]))
    r.setProbe(renderer.ProbeData(scenes.ambient_probe(size[0], size[1], 2.5)).BuildCDF())
    r.config = cfg
    r.launchParams.frame.c.x, r.launchParams.frame.c.y = size[0] // 2, size[1] // 2
    motion = r.motion_buffer()
    for k in range(2):                                        # the second step's motion vectors: every pixel reprojects onto itself
        r.launchParams.frame.subframe_index = k
        r.render()
        r.post(None, None, None, None, motion)
    g = r.temporal_gbuffer()
    color = r.post_buffers()[0]
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

    def first():
        r.variance_reset()
        r.variance(None, g, None, motion)

    cases = dict(VARIANCE_FIRST=first, VARIANCE_STEADY=lambda: r.variance(None, g, None, motion),
                 VFILTER=lambda: r.variance_filter(None, g, color), DENOISE=lambda: r.denoise(),
                 FIXED=lambda: r.expose(expose_fixed), RENDER=lambda: r.render_async())
    assert warmup >= r.variance_defaults().history_cap        # (VARIANCE_STEADY: the warm-up fills the history)
    ms = {k: [] for k in cases}
    shares = {}
    for _ in range(reps):                                     # alternately
        for k, fn in cases.items():
            ms[k].append(per_call(fn))
            if k.startswith("VARIANCE"):                      # what the timed calls did: the share of pixels below spatial_below
                n = r.downloadVariance()[0][..., 3]
                shares[k] = round(float((n < r.variance_defaults().spatial_below).mean()), 4)
    out = dict(config="C3", size=list(size), calls=calls, reps=reps, device=torch.cuda.get_device_name(0))
    for k, v in ms.items():
        out["ms_" + k] = round(float(np.median(v)), 4)
        out["spread_" + k] = [round(min(v), 4), round(max(v), 4)]
    for k in ("VARIANCE_FIRST", "VARIANCE_STEADY", "VFILTER"):
        out[k + "_over_DENOISE"] = round(out["ms_" + k] / out["ms_DENOISE"], 2)
    out["spatial_share"] = shares
    print(json.dumps(out), flush=True)
    r.close()


def quality(frames=12, size=(384, 216)):
    import reconstruct_ref as rr
    from temporal_common import _atrium, _path_view, quality_truth
    truth = quality_truth(size, frames)
    fill = rr.writers(size[0], size[1], (size[0] // 2, size[1] // 2), 30, 90, 0)[0]
    levels = (("periphery", 4), ("middle", 2), ("fovea", 1))
    rmse = lambda img: {name: round(float(np.sqrt(((img[..., :3].astype(np.float64) - truth[..., :3]) ** 2)[fill == fl].mean())), 6) for name, fl in levels}

    def run(stages, sigmas):
        c = abi.Config.reference_default()
        c.r_inner, c.r_outer = 30, 90
        c.spp_periphery, c.spp_middle, c.spp_fovea = 1, 2, 8
        r = _atrium(size, c)
        pc = r.post_defaults()
        pc.stages = stages
        motion = r.motion_buffer()
        for k in range(frames):
            _path_view(r, k, size)
            r.launchParams.frame.subframe_index = k
            r.render()
            r.post(pc, None, None, None, motion)
            if sigmas:
                r.variance(None, r.temporal_gbuffer(), None, motion)
        res = dict(post=rmse(r.downloadPostColor()))
        for s in sigmas:
            fc = r.variance_filter_defaults()
            fc.luminance_sigma = s
            r.variance_filter(fc, r.temporal_gbuffer(), r.post_buffers()[0])
            res["filter_sigma_%g" % s] = rmse(r.downloadVarianceFiltered()[0])
        r.close()
        return res

    base = abi.POST_RECONSTRUCT | abi.POST_TEMPORAL | abi.POST_MOTION
    out = dict(size=list(size), frames=frames, device=torch.cuda.get_device_name(0))
    res = run(base, (1.0, 2.0, 4.0, 8.0))
    out["rmse_post"] = res.pop("post")
    out.update({"rmse_post_" + k: v for k, v in res.items()})
    out["rmse_post_denoise"] = run(base | abi.POST_DENOISE, ())["post"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quality", action="store_true")
    args = ap.parse_args()
    if args.quality:
        quality()
    else:
        perf(args.calls, args.warmup, args.reps)
