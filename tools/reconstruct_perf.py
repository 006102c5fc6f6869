"""fovpt_gbuffer and fovpt_reconstruct at BASELINE C3 (262,144-triangle atrium, 1920 x 1080, radii 148 / 482, spp 1 / 2 / 8,
default configuration): device time per call from HIP events recorded on the library's stream around back-to-back calls (a
reconstruct builds its G-buffer, so it includes one), and the frame interval with and without a reconstruct after each frame.
Prints one JSON line.  Kernel statistics are a separate run:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/reconstruct_perf.py --calls 20
--sweep: the periphery / middle-ring RMSE gain (block-filled / reconstructed, and denoised / denoised + reconstructed, against
a 256-spp FOV_OFF render of the same view, 384 x 216) over support / depth_sigma / normal_sigma: how the defaults of
fovpt_reconstruct_defaults were chosen."""
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
    ms_rc = per_call(r.reconstruct)

    # the same window around frames alone and frames + reconstruct (frames issued back to back, as bench.py issues them)
    def frames(n, with_calls):
        r.synchronize()
        a.record(st)
        for _ in range(n):
            r.launchParams.frame.subframe_index = 0
            r.render_async()
            if with_calls:
                r.reconstruct()
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b) / n
    frames(5, False)
    f0, f1 = frames(40, False), frames(40, True)
    print(json.dumps(dict(config="C3", size=[1920, 1080], calls=calls, ms_per_gbuffer=round(ms_gb, 4),
                          ms_per_reconstruct=round(ms_rc, 4), ms_reconstruct_without_gbuffer=round(ms_rc - ms_gb, 4),
                          ms_per_frame=round(f0, 4), ms_per_frame_with_reconstruct=round(f1, 4),
                          device=torch.cuda.get_device_name(0))))
    r.close()


def sweep():
    import reconstruct_ref as rr
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
    r.denoise()
    den = r.downloadDenoisedColor()
    den_ptr = r.denoise_buffers()[0]
    fill, _, _, _ = rr.writers(size[0], size[1], (size[0] // 2, size[1] // 2), 30, 90, 0)
    rmse = lambda img, m: float(np.sqrt(((img[..., :3] - truth)[m] ** 2).mean()))
    for s in (1.0, 1.5, 2.0):
        for zs in (0.01, 0.05, 0.2, 1.0):
            for ns in (0.25, 0.5, 1.0):
                d = r.reconstruct_defaults()
                d.support, d.depth_sigma, d.normal_sigma = s, zs, ns
                r.reconstruct(d)
                rec = r.downloadReconstructedColor()
                r.reconstruct(d, den_ptr)
                den_rec = r.downloadReconstructedColor()
                print(json.dumps(dict(support=s, depth_sigma=zs, normal_sigma=ns,
                                      gain_periphery=round(rmse(raw, fill == 4) / rmse(rec, fill == 4), 4),
                                      gain_middle=round(rmse(raw, fill == 2) / rmse(rec, fill == 2), 4),
                                      gain_denoised_periphery=round(rmse(den, fill == 4) / rmse(den_rec, fill == 4), 4),
                                      gain_denoised_middle=round(rmse(den, fill == 2) / rmse(den_rec, fill == 2), 4))))
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    sweep() if args.sweep else perf(args.calls, args.warmup)
