"""fovpt_temporal at BASELINE C3 (262,144-triangle atrium, 1920 x 1080, radii 148 / 482, spp 1 / 2 / 8, default
configuration): device time per call from HIP events recorded on the library's stream around back-to-back calls.  A temporal
call traces its frame's G-buffer, so it includes one: ms_k_temporal is the call less a fovpt_gbuffer call.  Prints one JSON
line.  Kernel statistics are a separate run:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/temporal_perf.py --calls 20
--sweep: the periphery / middle-ring / fovea RMSE gain of render -> reconstruct -> temporal over render -> reconstruct on the
last frame of a 12-frame slow camera path (384 x 216 atrium, radii 30 / 90, spp 1 / 2 / 8, against a 256-spp FOV_OFF render
of the last view) over history caps and tolerances: how the defaults of fovpt_temporal_defaults were chosen (DESIGN.md,
section 12).
--motion: fovpt_temporal and fovpt_temporal_motion timed alternately in one process at C3, each step between its own pair of HIP
events on the library's stream (so an update issued before it is not counted): (a) nothing moved, (b) a quarter of the meshes
turned by 3 degrees and refitted from device pointers before every step (the motion of tools/refit_perf.py), (c) every mesh;
then, per scene of --scenes (c3, street), what the copy-on-first-write of the tracking adds to a fovpt_update_vertices call of
every mesh from device pointers: the same call timed in a context that only steps with fovpt_temporal (no tracking) and in one
that steps with fovpt_temporal_motion (every update is the first after a step, so it copies through the library's batched
kernel), and beside it the alternative, one device-to-device copy per mesh.  One JSON line each.
--motion-quality: the turning meshes of (b) at 384 x 216 under a still camera over 12 frames, render -> reconstruct -> temporal
with the defaults: RMSE of the periphery pixels on the turning meshes against a 256-spp render of the last pose, for
fovpt_reconstruct alone, fovpt_temporal and fovpt_temporal_motion."""
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


def _c3(size=(1920, 1080), radii=(148, 482), model=None, cam=None, probe=None):
    cfg = abi.Config.reference_default()
    cfg.r_inner, cfg.r_outer = radii
    cfg.spp_periphery, cfg.spp_middle, cfg.spp_fovea = 1, 2, 8
    cfg.write_guides = 1
    r = renderer.SampleRenderer(model if model is not None else scenes.atrium(262144))
    r.resize(size)
    cam = cam or scenes.ATRIUM_CAMERA
    r.setCamera(renderer.Camera(cam["eye"], cam["lookat"], cam["up"], cam["fovy"], size[0] / size[1]))
    r.setProbe(renderer.ProbeData(probe if probe is not None else scenes.ambient_probe(size[0], size[1], 2.5)).BuildCDF())
    r.config = cfg
    r.launchParams.frame.c.x, r.launchParams.frame.c.y = size[0] // 2, size[1] // 2
    return r


def _turned(v, deg):
    import numpy as np
    c = v.mean(axis=0, dtype=np.float64)
    a = np.deg2rad(deg)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    return ((v.astype(np.float64) - c) @ R.T + c).astype(np.float32)


def _timed(r, before, fn, calls, warmup):
    """Median over the calls of the device time of fn() alone, each after an untimed before(k)."""
    import numpy as np
    st = torch.cuda.ExternalStream(r.stream)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for k in range(warmup + calls):
        before(k)
        if k >= warmup:
            ev[k - warmup][0].record(st)
        fn()
        if k >= warmup:
            ev[k - warmup][1].record(st)
    r.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def motion_perf(calls, warmup, scene_names, rounds=3):
    import numpy as np
    r = _c3()
    size = (1920, 1080)
    r.render()
    model = r.model
    host = {k: np.ascontiguousarray(m.vertex, np.float32) for k, m in enumerate(model.meshes)}
    poses = [{k: torch.from_numpy(v if j == 0 else _turned(v, 3.0)).cuda() for k, v in host.items()} for j in range(2)]
    mo = r.motion_buffer()
    torch.cuda.synchronize()
    quarter = list(range(0, len(host), 4))
    cases = dict(a=[], b=quarter, c=list(host))
    out = dict(config="C3", size=list(size), calls=calls, rounds=rounds, meshes=len(host), device=torch.cuda.get_device_name(0))
    out["ms_gbuffer"] = round(_timed(r, lambda k: None, r.gbuffer, calls, warmup), 4)
    r.temporal_motion()                                   # tracking on for the whole comparison
    for name, moving in cases.items():
        before = (lambda k: None) if not moving else (lambda k: r.update_vertices({m: poses[k & 1][m] for m in moving}))
        res = dict(temporal=[], motion=[], motion_vectors=[])
        for _ in range(rounds):                           # alternately
            res["temporal"].append(_timed(r, before, r.temporal, calls, warmup))
            res["motion"].append(_timed(r, before, r.temporal_motion, calls, warmup))
            res["motion_vectors"].append(_timed(r, before, lambda: r.temporal_motion(None, None, None, None, mo), calls, warmup))
        for k, v in res.items():
            out["%s_ms_%s" % (name, k)] = round(float(np.median(v)), 4)
        out["%s_ratio_kernel" % name] = round((out["%s_ms_motion" % name] - out["ms_gbuffer"]) / (out["%s_ms_temporal" % name] - out["ms_gbuffer"]), 3)
    if quarter:
        r.update_vertices({m: poses[0][m] for m in host})
    print(json.dumps(out), flush=True)
    r.close()
    for name in scene_names:
        if name == "street":
            W, H = 2560, 1440
            model, cam, radii, probe = scenes.street(3800000), scenes.STREET_CAMERA, (197, 643), scenes.sky_probe(512, 256, seed=5)
        else:
            W, H = size
            model, cam, radii, probe = None, None, (148, 482), None
        res = dict(scene=name)
        for tracked in (False, True):
            q = _c3((W, H), radii, model, cam, probe)
            q.render()
            dev = {k: torch.from_numpy(np.ascontiguousarray(m.vertex, np.float32)).cuda() for k, m in enumerate(q.model.meshes)}
            torch.cuda.synchronize()
            step = q.temporal_motion if tracked else q.temporal
            step()
            ms = [_timed(q, lambda k: step(), lambda: q.update_vertices(dev), calls, warmup) for _ in range(rounds)]
            res["update_ms_tracked" if tracked else "update_ms_untracked"] = round(float(np.median(ms)), 4)
            res["meshes"], res["vertices"] = len(dev), int(sum(v.shape[0] for v in dev.values()))
            if tracked:
                # the alternative to the batched kernel: one device-to-device copy per mesh on the same stream
                dst = {k: torch.empty_like(v) for k, v in dev.items()}
                torch.cuda.synchronize()

                def copies():
                    with torch.cuda.stream(torch.cuda.ExternalStream(q.stream)):
                        for k, v in dev.items():
                            dst[k].copy_(v, non_blocking=True)
                res["memcpy_per_mesh_ms"] = round(_timed(q, lambda k: None, copies, calls, warmup), 4)
            q.close()
        res["copy_on_first_write_ms"] = round(res["update_ms_tracked"] - res["update_ms_untracked"], 4)
        print(json.dumps(res), flush=True)


def motion_quality(frames=12, size=(384, 216)):
    import numpy as np
    import reconstruct_ref as rr
    model = scenes.atrium(262144)
    nm = len(model.meshes)
    moving = list(range(0, nm, 4))
    pose = {k: np.ascontiguousarray(model.meshes[k].vertex, np.float32) for k in moving}
    seq = []
    for _ in range(frames):
        pose = {k: _turned(v, 3.0) for k, v in pose.items()}
        seq.append(pose)
    cfg = abi.Config.reference_default()
    cfg.uniform, cfg.spp_uniform = 1, 256
    t = _c3(size, (30, 90), model)
    t.config = cfg
    t.update_vertices(seq[-1])
    t.render()
    truth = t.downloadAccum()
    prim = t.downloadGBuffer()["prim"]
    t.close()
    mesh_of = np.concatenate([np.full(len(m.index), k) for k, m in enumerate(model.meshes)])
    on_moving = (prim != rr.MISS) & np.isin(mesh_of[np.where(prim == rr.MISS, 0, prim).astype(np.int64)], moving)
    fill = rr.writers(size[0], size[1], (size[0] // 2, size[1] // 2), 30, 90, 0)[0]
    sel = on_moving & (fill == 4)
    rmse = lambda img: float(np.sqrt(((img[..., :3].astype(np.float64) - truth[..., :3]) ** 2)[sel].mean()))
    out = dict(size=list(size), frames=frames, moving_meshes=len(moving), pixels=int(sel.sum()))
    for name in ("temporal", "temporal_motion"):
        r = _c3(size, (30, 90), model)
        for k in range(frames):
            r.update_vertices(seq[k])
            r.render()
            r.reconstruct()
            getattr(r, name)(None, r.reconstruct_buffers()[0])
        tem, n = r.downloadTemporalColor(), r.downloadTemporalHistory()[..., 3]
        out["rmse_reconstruct"] = round(rmse(r.downloadReconstructedColor()), 6)
        out["rmse_" + name] = round(rmse(tem), 6)
        out["mean_history_" + name] = round(float(n[sel].mean()), 3)
        r.close()
    print(json.dumps(out), flush=True)


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
    ap.add_argument("--motion", action="store_true")
    ap.add_argument("--motion-quality", action="store_true")
    ap.add_argument("--scenes", default="c3,street", help="--motion: the scenes of the update-cost part (c3, street, or none)")
    args = ap.parse_args()
    if args.motion:
        motion_perf(args.calls, args.warmup, [s_ for s_ in args.scenes.split(",") if s_ and s_ != "none"])
    elif args.motion_quality:
        motion_quality()
    else:
        sweep() if args.sweep else perf(args.calls, args.warmup)
