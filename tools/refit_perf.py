"""fovpt_update_vertices at BASELINE C3 (262,144-triangle atrium, 1920 x 1080, radii 148 / 482, spp 1 / 2 / 8) and on the
3.8 M-triangle street (C4's 2560 x 1440, radii 197 / 643): device time of one refit of every mesh from device pointers and from
host arrays (HIP events on the library's stream around back-to-back calls, after a warm-up), and the time of one
FOVPT_UPDATE_REBUILD (host-synchronous: wall clock, and the build's own stats.ms_bvh_build).
Quality: a quarter of the meshes turn about their centres by 3 degrees per frame for --frames frames, refit after each; then
tools/bvhstat.py's SAH cost and the frame time of the refit tree against the same geometry rebuilt.  Prints one JSON line per
scene.  Kernel statistics are a separate run:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/refit_perf.py --scenes c3 --calls 20 --frames 0"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import refit_ref as rf  # noqa: E402
from fovpathtracing_optixcodelatest_amd import abi, renderer, scenes  # noqa: E402

SCENES = {
    "c3": dict(make=lambda: scenes.atrium(262144), cam=scenes.ATRIUM_CAMERA, size=(1920, 1080), radii=(148, 482), probe="ambient"),
    "street": dict(make=lambda: scenes.street(3800000), cam=scenes.STREET_CAMERA, size=(2560, 1440), radii=(197, 643), probe="sky"),
}


def nodes_of(r):
    p, n = C.c_void_p(), C.c_size_t()
    r._check(r._L.fovpt_debug_buffer(r._ctx, b"bvh_nodes", C.byref(p), C.byref(n)))
    return r.download(p.value, np.empty(n.value // 4, np.uint32)).reshape(-1, 32)


def device_ms(r, fn, calls, warmup):
    for _ in range(warmup):
        fn()
    r.synchronize()
    st = torch.cuda.ExternalStream(r.stream)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    host = (time.perf_counter() - t) / calls
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b) / calls, host * 1e3


def frame_ms(r, frames=20):
    def one():
        r.launchParams.frame.subframe_index = 0
        r.render()
    for _ in range(3):
        one()
    ts = []
    for _ in range(frames):
        t = time.perf_counter()
        one()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts) * 1e3)


def turn(v, deg):
    c = v.mean(axis=0, dtype=np.float64)
    a = np.deg2rad(deg)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    return ((v.astype(np.float64) - c) @ R.T + c).astype(np.float32)


def run(name, calls, warmup, frames):
    S = SCENES[name]
    model = S["make"]()
    W, H = S["size"]
    r = renderer.SampleRenderer(model)
    r.resize(S["size"])
    cam = S["cam"]
    r.setCamera(renderer.Camera(cam["eye"], cam["lookat"], cam["up"], cam["fovy"], W / H))
    probe = scenes.ambient_probe(W, H, 2.5) if S["probe"] == "ambient" else scenes.sky_probe(512, 256, seed=5)
    r.setProbe(renderer.ProbeData(probe).BuildCDF())
    cfg = abi.Config.reference_default()
    cfg.r_inner, cfg.r_outer = S["radii"]
    cfg.spp_periphery, cfg.spp_middle, cfg.spp_fovea = 1, 2, 8
    r.config = cfg
    r.launchParams.frame.c.x, r.launchParams.frame.c.y = W // 2, H // 2
    r.render()
    st0 = r.stats()
    host = {k: np.ascontiguousarray(m.vertex, np.float32) for k, m in enumerate(model.meshes)}
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    torch.cuda.synchronize()
    out = dict(scene=name, triangles=model.num_triangles, meshes=len(model.meshes), bvh_nodes=int(st0.num_bvh_nodes),
               levels=len(rf.levels_of(nodes_of(r))) - 1, build_ms=round(st0.ms_bvh_build, 3),
               vertices=int(sum(v.shape[0] for v in host.values())))
    out["refit_device_ms"], out["refit_device_call_host_ms"] = (round(x, 4) for x in device_ms(r, lambda: r.update_vertices(dev), calls, warmup))
    out["refit_host_upload_ms"], out["refit_host_call_host_ms"] = (round(x, 4) for x in device_ms(r, lambda: r.update_vertices(host), calls, warmup))
    t = time.perf_counter()
    r.update_vertices({}, rebuild=True)
    out["rebuild_wall_ms"] = round((time.perf_counter() - t) * 1e3, 3)
    out["rebuild_build_ms"] = round(r.stats().ms_bvh_build, 3)
    if frames:
        moving = list(range(0, len(model.meshes), 4))
        cur = dict(host)
        base_nodes = nodes_of(r)
        out["frame_ms_built"] = round(frame_ms(r), 4)
        for _ in range(frames):
            cur.update({k: turn(cur[k], 3.0) for k in moving})
            r.update_vertices({k: cur[k] for k in moving})
        refit_nodes = nodes_of(r)
        out["frame_ms_refit_after_%d" % frames] = round(frame_ms(r), 4)
        r.update_vertices({}, rebuild=True)
        rebuilt_nodes = nodes_of(r)
        out["frame_ms_rebuilt_after_%d" % frames] = round(frame_ms(r), 4)
        out["sah_built"] = round(rf.sah_cost(base_nodes, rf.levels_of(base_nodes)), 3)
        out["sah_refit"] = round(rf.sah_cost(refit_nodes, rf.levels_of(refit_nodes)), 3)
        out["sah_rebuilt"] = round(rf.sah_cost(rebuilt_nodes, rf.levels_of(rebuilt_nodes)), 3)
        out["moving_meshes"] = len(moving)
    r.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c3,street")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=60)
    a = ap.parse_args()
    for s in a.scenes.split(","):
        run(s, a.calls, a.warmup, a.frames)


if __name__ == "__main__":
    main()
