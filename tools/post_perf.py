"""fovpt_post against the entry points it stands for at BASELINE C3 (262,144-triangle atrium, 1920 x 1080, radii 148 / 482,
spp 1 / 2 / 8, default configurations): device time per call from HIP events recorded on the library's stream around --calls
calls back to back after a warm-up.  In one process, alternately, --reps times each:
    G    fovpt_gbuffer
    A    fovpt_reconstruct followed by fovpt_temporal_motion (of the reconstruction's colour, with motion vectors)
    B    fovpt_post with RECONSTRUCT | TEMPORAL | MOTION (with motion vectors)
    DA   fovpt_denoise, then A on the denoised colour
    DB   fovpt_post with DENOISE | RECONSTRUCT | TEMPORAL | MOTION
and prints one JSON line: the median over the repetitions and the spread (min, max) of each, and whether B <= A - 0.9 G (one
G-buffer trace less, with a tenth of it as allowance for timing spread).  Kernel statistics are a
separate run:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/post_perf.py --calls 20 --reps 1"""
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
    mo = r.motion_buffer()
    rec, den = r.reconstruct_buffers()[0], r.denoise_buffers()[0]
    pc = r.post_defaults()
    pcd = r.post_defaults()
    pcd.stages |= abi.POST_DENOISE
    r.temporal_motion()                                       # tracking on, a history to reproject, for every case alike

    def separate(in_color=None):
        r.reconstruct(None, in_color)
        r.temporal_motion(None, rec, None, None, mo)

    def denoise_separate():
        r.denoise()
        separate(den)

    cases = dict(G=r.gbuffer, A=separate, B=lambda: r.post(pc, None, None, None, mo), DA=denoise_separate,
                 DB=lambda: r.post(pcd, None, None, None, mo))
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
    out["A_minus_0.9G"] = round(med["A"] - 0.9 * med["G"], 4)
    out["B_within_bound"] = bool(med["B"] <= med["A"] - 0.9 * med["G"])
    out["DB_within_bound"] = bool(med["DB"] <= med["DA"] - 0.9 * med["G"])
    out["spread_A_over_0.1G"] = round((max(ms["A"]) - min(ms["A"])) / (0.1 * med["G"]), 3)
    print(json.dumps(out), flush=True)
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    main(args.calls, args.warmup, args.reps)
