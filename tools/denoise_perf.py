"""fovpt_denoise at BASELINE C3 (262,144-triangle atrium, 1920 x 1080, radii 148 / 482, spp 1 / 2 / 8, default denoiser
configuration): device time per call from HIP events recorded on the library's stream around back-to-back calls.  Prints one
JSON line.  Kernel statistics are a separate run:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/denoise_perf.py --calls 20
--sweep: the periphery / middle-ring RMSE gain (raw / denoised, against a 256-spp FOV_OFF render of the same view, 384 x 216)
for a grid of edge-stopping scales: how the defaults of fovpt_denoise_defaults were chosen (denoiser)."""
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


def make(size, cfg, tris, probe=(96, 54)):
    cfg.write_guides = 1
    r = renderer.SampleRenderer(scenes.atrium(tris))
    r.resize(size)
    r.setCamera(renderer.Camera(scenes.ATRIUM_CAMERA["eye"], scenes.ATRIUM_CAMERA["lookat"], scenes.ATRIUM_CAMERA["up"],
                                scenes.ATRIUM_CAMERA["fovy"], size[0] / size[1]))
    r.setProbe(renderer.ProbeData(scenes.ambient_probe(probe[0], probe[1], 2.5)).BuildCDF())
    r.config = cfg
    r.launchParams.frame.c.x, r.launchParams.frame.c.y = size[0] // 2, size[1] // 2
    return r


def fov(ri, ro, spp=(1, 2, 8)):
    c = abi.Config.reference_default()
    c.r_inner, c.r_outer = ri, ro
    c.spp_periphery, c.spp_middle, c.spp_fovea = spp
    return c


def perf(calls, warmup):
    r = make((1920, 1080), fov(148, 482), 262144, probe=(1920, 1080))
    r.render()
    st = torch.cuda.ExternalStream(r.stream)
    for _ in range(warmup):
        r.denoise()
    r.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    for _ in range(calls):
        r.denoise()
    b.record(st)
    b.synchronize()
    ms = a.elapsed_time(b) / calls
    # the same window around frames alone and frames + denoise (frames issued back to back, as bench.py issues them)
    def frames(n, with_denoise):
        r.synchronize()
        a.record(st)
        for _ in range(n):
            r.launchParams.frame.subframe_index = 0
            r.render_async()
            if with_denoise:
                r.denoise()
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b) / n
    frames(5, False)
    f0, f1 = frames(40, False), frames(40, True)
    npix = 1920 * 1080
    print(json.dumps(dict(config="C3", size=[1920, 1080], calls=calls, ms_per_denoise=round(ms, 4),
                          ms_per_frame=round(f0, 4), ms_per_frame_with_denoise=round(f1, 4),
                          guide_bytes_per_iteration=npix * 48, device=torch.cuda.get_device_name(0))))
    r.close()


def sweep():
    import denoise_ref as dn
    size = (384, 216)
    t = make(size, abi.Config.reference_default(), 8000)
    c = t.config
    c.uniform, c.spp_uniform = 1, 256
    t.config = c
    t.render()
    truth = t.downloadAccum()[..., :3].astype(np.float64)
    t.close()
    cfg = fov(30, 90)
    r = make(size, cfg, 8000)
    r.render()
    raw = r.downloadAccum()[..., :3]
    _, pas = dn.level_map(size[0], size[1], (size[0] // 2, size[1] // 2), 30, 90, 0)
    rmse = lambda img, m: float(np.sqrt(((img[..., :3] - truth)[m] ** 2).mean()))
    for cs in (1.0, 2.0, 4.0, 8.0, 16.0):
        for ns in (0.25, 0.5, 1.0):
            for as_ in (0.05, 0.1, 0.2):
                d = r.denoise_defaults()
                d.color_sigma, d.normal_sigma, d.albedo_sigma = cs, ns, as_
                r.denoise(d)
                den = r.downloadDenoisedColor()
                print(json.dumps(dict(color_sigma=cs, normal_sigma=ns, albedo_sigma=as_,
                                      gain_periphery=round(rmse(raw, pas == 0) / rmse(den, pas == 0), 3),
                                      gain_middle=round(rmse(raw, pas == 1) / rmse(den, pas == 1), 3))))
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    sweep() if args.sweep else perf(args.calls, args.warmup)
