"""fovpt_temporal at BASELINE C3 (262,144-triangle atrium, 1920 x 1080, radii 148 / 482, spp 1 / 2 / 8, default
configuration): device time per call from HIP events recorded on the library's stream around back-to-back calls.  A temporal
call traces its frame's G-buffer, so it includes one: ms_k_temporal is the call less a fovpt_gbuffer call.  Prints one JSON
line.  Kernel statistics are a separate run:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/temporal_perf.py --calls 20
--sweep: the periphery / middle-ring / fovea RMSE gain of render -> reconstruct -> temporal over render -> reconstruct on the
last frame of a 12-frame slow camera path (384 x 216 atrium, radii 30 / 90, spp 1 / 2 / 8, against a 256-spp FOV_OFF render
of the last view) over history caps and tolerances: how the defaults of fovpt_temporal_defaults were chosen (DESIGN.md,
section 12)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from fovpathtracing_optixcodelatest_amd import abi, renderer, scenes  # noqa: E402


def perf(calls, warmup):
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
    ms_gb = per_call(r.gbuffer)
    ms_tp = per_call(r.temporal)
    print(json.dumps(dict(config="C3", size=list(size), calls=calls, ms_per_gbuffer=round(ms_gb, 4),
                          ms_per_temporal=round(ms_tp, 4), ms_k_temporal=round(ms_tp - ms_gb, 4),
                          device=torch.cuda.get_device_name(0))))
    r.close()


def sweep():
    from temporal_common import quality_run, quality_truth
    truth = quality_truth()
    grid = []
    for cp in (2, 4, 8, 16, 32):
        for nt in (0.05, 0.1, 0.3):
            for zt in (0.01, 0.02, 0.05):
                grid.append(dict(history_periphery=cp, normal_tolerance=nt, depth_tolerance=zt))
    grid += [dict(history_middle=cm) for cm in (1, 2, 4, 8, 16)] + [dict(history_fovea=cf) for cf in (1, 2, 4)]
    for d, res in zip(grid, quality_run(configs=grid, truth=truth)):
        print(json.dumps(dict(d, **{"gain_" + k: round(a / b, 4) for k, (a, b) in res.items()},
                              **{"rmse_" + k: round(b, 6) for k, (a, b) in res.items()})))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    sweep() if args.sweep else perf(args.calls, args.warmup)
