"""fovpt_warp at BASELINE C3 (262,144-triangle atrium, 1920 x 1080, radii 148 / 482, spp 1 / 2 / 8): device time per call from
HIP events recorded on the library's stream around --calls calls back to back after a warm-up.  For a small slide, a turn and a
dolly-in of the camera, in one process, alternately, --reps times each:
    WARP_G  fovpt_warp with a caller's G-buffer (fovpt_temporal_gbuffer's, of the fovpt_post step): clear, k_warp_scatter, k_warp_resolve
    WARP_T  fovpt_warp with its own trace: the G-buffer's three launches first
    FIXED   fovpt_expose FIXED: the yardstick of a plain full-frame pass (reads 16 bytes, writes 20 per pixel)
    RENDER  one fovpt_render: the frame the warp stands in for
both images from the accum / frame buffer into the renderer's own buffers, fill_radius 2, and prints one JSON line: per motion the
median over the repetitions and the spread (min, max) of each, and the shares of the three classes.  Nothing here is a threshold
(DESIGN.md, section 21).  Kernel statistics are a separate run:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/warp_perf.py --calls 20 --reps 1
--motion: fovpt_warp and fovpt_warp_motion at C3 with a share of the atrium's meshes moving each frame (none, a quarter, all: turned
by 3 degrees and refitted from device pointers, the motion of tools/refit_perf.py and tools/temporal_perf.py --motion).  Per share:
update -> render -> post (MOTION) once, then, for a small slide of the camera and advance 1, in one process, alternately, --reps times
each, --calls calls back to back:
    WARP_G / MOTION_G  fovpt_warp / fovpt_warp_motion with the post step's G-buffer (fovpt_temporal_gbuffer) and hit records
    WARP_T / MOTION_T  the two with the call's own trace
and prints one JSON line: per share the medians and spreads, the share of source pixels on moved meshes, and the direct / filled /
empty shares of both calls."""
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
    r.post()
    g = r.temporal_gbuffer()                                  # the rendered frame's: the camera does not move below
    (ex, ey, ez), (lx, ly, lz) = cam["eye"], cam["lookat"]
    motions = dict(slide=((ex, ey, ez + 20.0), (lx, ly, lz + 20.0)), turn=((ex, ey, ez), (lx, ly, lz + 150.0)), dolly_in=((ex + 100.0, ey, ez), (lx, ly, lz)))
    fixed = r.expose_defaults()
    fixed.mode = abi.EXPOSE_FIXED
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

    out = dict(config="C3", size=list(size), calls=calls, reps=reps, device=torch.cuda.get_device_name(0), fill_radius=r.warp_defaults().fill_radius)
    n = size[0] * size[1]
    for name, (eye, lookat) in motions.items():
        to = r.warp_camera(renderer.Camera(eye, lookat, cam["up"], cam["fovy"], size[0] / size[1]))
        cases = dict(WARP_G=lambda: r.warp(to, None, g), WARP_T=lambda: r.warp(to), FIXED=lambda: r.expose(fixed), RENDER=lambda: r.render_async())
        ms = {k: [] for k in cases}
        for _ in range(reps):                                 # alternately
            for k, fn in cases.items():
                ms[k].append(per_call(fn))
        r.warp(to, None, g)
        c = r.warp_counts()
        res = dict(shares=dict(direct=round(c.direct / n, 4), filled=round(c.filled / n, 4), empty=round(c.empty / n, 4), splatted=round(c.splatted / n, 4)))
        for k, v in ms.items():
            res["ms_" + k] = round(float(np.median(v)), 4)
            res["spread_" + k] = [round(min(v), 4), round(max(v), 4)]
        res["WARP_G_over_FIXED"] = round(res["ms_WARP_G"] / res["ms_FIXED"], 3)
        res["RENDER_over_WARP_G"] = round(res["ms_RENDER"] / res["ms_WARP_G"], 1)
        out[name] = res
    print(json.dumps(out), flush=True)
    r.close()


def motion(calls, warmup, reps):
    size = (1920, 1080)
    cfg = abi.Config.reference_default()
    cfg.r_inner, cfg.r_outer = 148, 482
    cfg.spp_periphery, cfg.spp_middle, cfg.spp_fovea = 1, 2, 8
    cfg.write_guides = 1
    model = scenes.atrium(262144)
    r = renderer.SampleRenderer(model)
    r.resize(size)
    cam = scenes.ATRIUM_CAMERA
    r.setCamera(renderer.Camera(cam["eye"], cam["lookat"], cam["up"], cam["fovy"], size[0] / size[1]))
    r.setProbe(renderer.ProbeData(scenes.ambient_probe(size[0], size[1], 2.5)).BuildCDF())
    r.config = cfg
    r.launchParams.frame.c.x, r.launchParams.frame.c.y = size[0] // 2, size[1] // 2

    def turned(v, deg):
        c = v.mean(axis=0, dtype=np.float64)
        a = np.deg2rad(deg)
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        return ((v.astype(np.float64) - c) @ R.T + c).astype(np.float32)

    host = {k: np.ascontiguousarray(m.vertex, np.float32) for k, m in enumerate(model.meshes)}
    poses = [{k: torch.from_numpy(v if j == 0 else turned(v, 3.0)).cuda() for k, v in host.items()} for j in range(2)]
    torch.cuda.synchronize()
    mesh_of = np.concatenate([np.full(len(m.index), k) for k, m in enumerate(model.meshes)])
    (ex, ey, ez), (lx, ly, lz) = cam["eye"], cam["lookat"]
    to = r.warp_camera(renderer.Camera((ex, ey, ez + 20.0), (lx, ly, lz + 20.0), cam["up"], cam["fovy"], size[0] / size[1]))
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

    n = size[0] * size[1]
    mc = r.warp_motion_defaults()
    out = dict(config="C3", size=list(size), calls=calls, reps=reps, meshes=len(host), device=torch.cuda.get_device_name(0),
               fill_radius=mc.fill_radius, advance=mc.advance)
    r.render()
    r.post()                                                  # tracking on
    for name, moving in (("none", []), ("quarter", list(range(0, len(host), 4))), ("all", list(host))):
        if moving:
            r.update_vertices({m: poses[1][m] for m in moving})
        r.render()
        r.post()
        g = r.temporal_gbuffer()
        prim = r.downloadGBuffer(g)["prim"]
        hit = prim != 0xffffffff
        on_moved = hit & np.isin(mesh_of[np.where(hit, prim, 0).astype(np.int64)], moving)
        cases = dict(WARP_G=lambda: r.warp(to, None, g), MOTION_G=lambda: r.warp_motion(to, mc, g), WARP_T=lambda: r.warp(to),
                     MOTION_T=lambda: r.warp_motion(to, mc))
        ms = {k: [] for k in cases}
        for _ in range(reps):                                 # alternately
            for k, fn in cases.items():
                ms[k].append(per_call(fn))
        res = dict(moving_meshes=len(moving), moved_sources=round(float(on_moved.sum()) / n, 4))
        for k, call in (("warp", cases["WARP_G"]), ("warp_motion", cases["MOTION_G"])):
            call()
            c = r.warp_counts()
            res["shares_" + k] = dict(direct=round(c.direct / n, 4), filled=round(c.filled / n, 4), empty=round(c.empty / n, 4), splatted=round(c.splatted / n, 4))
        for k, v in ms.items():
            res["ms_" + k] = round(float(np.median(v)), 4)
            res["spread_" + k] = [round(min(v), 4), round(max(v), 4)]
        res["MOTION_G_over_WARP_G"] = round(res["ms_MOTION_G"] / res["ms_WARP_G"], 3)
        res["MOTION_T_minus_WARP_T"] = round(res["ms_MOTION_T"] - res["ms_WARP_T"], 4)
        out[name] = res
        if moving:                                            # back where they were, and an interval without motion
            r.update_vertices({m: poses[0][m] for m in moving})
            r.render()
            r.post()
    print(json.dumps(out), flush=True)
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--motion", action="store_true", help="fovpt_warp_motion against fovpt_warp with moving meshes")
    args = ap.parse_args()
    (motion if args.motion else main)(args.calls, args.warmup, args.reps)
