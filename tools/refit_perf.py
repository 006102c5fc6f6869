"""fovpt_update_vertices at BASELINE C3 (262,144-triangle atrium, 1920 x 1080, radii 148 / 482, spp 1 / 2 / 8) and on the
3.8 M-triangle street (C4's 2560 x 1440, radii 197 / 643): device time of one refit of every mesh from device pointers and from
host arrays (HIP events on the library's stream around back-to-back calls, after a warm-up), and the time of one
FOVPT_UPDATE_REBUILD (host-synchronous: wall clock, and the build's own stats.ms_bvh_build).
Quality: a quarter of the meshes turn about their centres by 3 degrees per frame for --frames frames, refit after each; then
tools/bvhstat.py's SAH cost and the frame time of the refit tree against the same geometry rebuilt.  Prints one JSON line per
scene.  Kernel statistics are a separate run:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/refit_perf.py --scenes c3 --calls 20 --frames 0

--transforms: fovpt_update_transforms and fovpt_hierarchy_cost instead.  On one context, every mesh moved, --rounds rounds of
update_transforms and update_vertices with device pointers in turn (ms per call, device time), first while nobody watches the
cost and then, after the context's first hierarchy_cost(), with a measurement behind every refit: what a measurement costs is
the difference (its kernels' own times: the kernel-trace run above with --transforms).  Then the quality experiment with the
device's current / built ratio polled after every frame's refit, beside the frame times.

--skin: fovpt_update_skinned instead.  Every mesh gets a procedural skin of 2 .. 64 joints (skin_ref.bend) and one pose; on one
context, --rounds rounds of three updates to the same positions in turn: update_skinned with host matrices, update_vertices with
device pointers to the positions skinned beforehand, update_vertices with the same positions as host arrays (ms per call, device
time on the library's stream; the median over the rounds and every round).

--morph: fovpt_update_morphed instead.  Every mesh gets --morph-dense dense and --morph-sparse sparse procedural targets
(morph_ref.bumps; a sparse one lists --morph-fraction of the mesh's vertices) and one pose with --morph-active weights that are
not zero; the mix is recorded in the output.  On one context, --rounds rounds of three updates to the same positions in turn:
update_morphed with host weights, update_vertices with device pointers to the positions morphed beforehand, update_vertices with
the same positions as host arrays.  Then every mesh gets --skin's skin as well, and update_morphed with weights and matrices
alternates with update_skinned of the same matrices.

--rig: fovpt_update_animated instead.  Every mesh gets --skin's skin and is bound to a rig of 1024 nodes (8 levels, a rotation
channel of four keys on every node, one clip).  On one context, --rounds rounds of three updates to the same positions in turn:
update_animated, update_skinned with host palettes computed beforehand (rig_ref.pose), update_vertices with device pointers.
Then, on a scene of a few vertices, k_rig_pose by itself for 64 and 1024 nodes, flat and as one chain: what update_animated
takes beyond update_skinned with a device palette, which issues the same launches but for k_rig_pose.

--async: FOVPT_UPDATE_REBUILD_ASYNC against FOVPT_UPDATE_REBUILD.  The quality experiment's motion (a quarter of the meshes turning
3 degrees per frame), frames back to back with two in flight (the loop waits for frame f - 2 before it issues frame f, as an
application's present would; nothing else waits), the cost polled after every frame and a rebuild asked for whenever
current / built exceeds --threshold.  In one run, --rounds times in turn: a loop of --frames frames that rebuilds synchronously
(the reference) and one that passes the new flag.  Per loop: the mean, median and longest frame interval (device events on the
library's stream behind every frame), the longest and median host time of every kind of call, and for the new flag the longest
host time of any call while a build runs, the time from request to READY, the build's device time on its own stream, the mean
interval while a build runs against the interval otherwise, and the intervals of the frames whose update adopted.  Last, on an
idle device: the device and host time of one adoption, and the host time of the poll that releases the retired hierarchy."""
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


def make_renderer(name):
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
    return model, r


def run(name, calls, warmup, frames):
    model, r = make_renderer(name)
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


def turn_matrix(v, deg):
    """turn() as a row-major 3 x 4 matrix."""
    c = v.mean(axis=0, dtype=np.float64)
    a = np.deg2rad(deg)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    return np.concatenate([R, (c - R @ c)[:, None]], axis=1).astype(np.float32)


def run_transforms(name, calls, warmup, frames, rounds):
    import transform_ref as tf
    model, r = make_renderer(name)
    st0 = r.stats()
    ts = {k: turn_matrix(m.vertex, 3.0) for k, m in enumerate(model.meshes)}
    dev = {k: torch.from_numpy(v).cuda() for k, v in tf.restate(model, ts).items()}
    torch.cuda.synchronize()
    out = dict(scene=name, triangles=model.num_triangles, meshes=len(model.meshes), bvh_nodes=int(st0.num_bvh_nodes),
               vertices=int(sum(m.vertex.shape[0] for m in model.meshes)), rounds=rounds, calls=calls)
    t_ms = {False: [], True: []}
    v_ms = {False: [], True: []}
    for watching in (False, True):
        if watching:
            r.hierarchy_cost()                                  # from here on a measurement follows every refit
        for _ in range(rounds):
            t_ms[watching].append(device_ms(r, lambda: r.update_transforms(ts), calls, warmup)[0])
            v_ms[watching].append(device_ms(r, lambda: r.update_vertices(dev), calls, warmup)[0])
    med = lambda x: float(np.median(x))
    out["update_transforms_ms"] = round(med(t_ms[False]), 4)
    out["update_vertices_device_ms"] = round(med(v_ms[False]), 4)
    out["update_transforms_ms_rounds"] = [round(x, 4) for x in t_ms[False]]
    out["update_vertices_device_ms_rounds"] = [round(x, 4) for x in v_ms[False]]
    out["update_transforms_watched_ms"] = round(med(t_ms[True]), 4)
    out["update_vertices_device_watched_ms"] = round(med(v_ms[True]), 4)
    out["cost_measurement_ms"] = round(0.5 * (med(t_ms[True]) - med(t_ms[False]) + med(v_ms[True]) - med(v_ms[False])), 4)
    c = r.hierarchy_cost(wait=True)
    out["measured_of_updates"] = [int(c.measured), int(c.updates)]
    t = time.perf_counter()
    for _ in range(20):
        r.hierarchy_cost()
    out["poll_host_us"] = round((time.perf_counter() - t) / 20 * 1e6, 2)
    if frames:
        # the quality experiment of run(), the motion sent as matrices: turn k of a moving mesh is 3 (k + 1) degrees from rest
        r.update_transforms({k: np.eye(3, 4, dtype=np.float32) for k in range(len(model.meshes))}, rebuild=True)
        moving = list(range(0, len(model.meshes), 4))
        out["frame_ms_built"] = round(frame_ms(r), 4)
        ratios, lag = [], 0
        for f in range(frames):
            r.update_transforms({k: turn_matrix(model.meshes[k].vertex, 3.0 * (f + 1)) for k in moving})
            r.launchParams.frame.subframe_index = 0
            r.render_async()
            c = r.hierarchy_cost()                              # the caller's poll: never waits
            lag = max(lag, int(c.updates - c.measured))
            ratios.append(c.current / c.built)
        c = r.hierarchy_cost(wait=True)
        ratios.append(c.current / c.built)
        out["cost_ratio_every_10_frames"] = [round(x, 3) for x in ratios[9::10]]
        out["cost_ratio_final"] = round(ratios[-1], 3)
        out["cost_built"], out["cost_current"] = round(c.built, 3), round(c.current, 3)
        out["poll_lag_max_updates"] = lag
        nodes = nodes_of(r)
        out["sah_refit_host"] = round(rf.sah_cost(nodes, rf.levels_of(nodes)), 3)
        out["frame_ms_refit_after_%d" % frames] = round(frame_ms(r), 4)
        r.update_transforms({}, rebuild=True)
        out["frame_ms_rebuilt_after_%d" % frames] = round(frame_ms(r), 4)
        out["cost_rebuilt"] = round(r.hierarchy_cost().built, 3)
        out["moving_meshes"] = len(moving)
    r.close()
    print(json.dumps(out), flush=True)


def run_skin(name, calls, warmup, rounds):
    import skin_ref as sk
    model, r = make_renderer(name)
    st0 = r.stats()
    skins = {k: sk.bend(m.vertex, 2 + (7 * k) % 63) for k, m in enumerate(model.meshes)}
    poses = {k: sk.bend_pose(m.vertex, skins[k][2], 12.0, (0.0, 0.02 * (k % 5), 0.0)) for k, m in enumerate(model.meshes)}
    t = time.perf_counter()
    r.set_skins(skins)
    set_skins_ms = (time.perf_counter() - t) * 1e3
    host = sk.restate(model, skins, poses)
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    torch.cuda.synchronize()
    out = dict(scene=name, triangles=model.num_triangles, meshes=len(model.meshes), bvh_nodes=int(st0.num_bvh_nodes),
               vertices=int(sum(m.vertex.shape[0] for m in model.meshes)), joints=int(sum(s[2] for s in skins.values())),
               rounds=rounds, calls=calls, set_skins_host_ms=round(set_skins_ms, 3))
    ms = dict(update_skinned=[], update_vertices_device=[], update_vertices_host=[])
    host_ms = dict(update_skinned=[], update_vertices_device=[], update_vertices_host=[])
    fns = dict(update_skinned=lambda: r.update_skinned(poses), update_vertices_device=lambda: r.update_vertices(dev),
               update_vertices_host=lambda: r.update_vertices(host))
    for _ in range(rounds):
        for k, fn in fns.items():
            d, h = device_ms(r, fn, calls, warmup)
            ms[k].append(d)
            host_ms[k].append(h)
    for k in fns:
        out[k + "_ms"] = round(float(np.median(ms[k])), 4)
        out[k + "_ms_rounds"] = [round(x, 4) for x in ms[k]]
        out[k + "_host_ms"] = round(float(np.median(host_ms[k])), 4)
    # the three leave the same positions behind
    p, n = C.c_void_p(), C.c_size_t()
    r._check(r._L.fovpt_debug_buffer(r._ctx, b"scene_vertices", C.byref(p), C.byref(n)))
    r.update_skinned(poses)
    got = r.download(p.value, np.empty(n.value // 4, np.uint32))
    out["positions_match_restatement"] = bool(np.array_equal(got, np.concatenate([host[k] for k in range(len(model.meshes))]).view(np.uint32).reshape(-1)))
    r.close()
    print(json.dumps(out), flush=True)


def alternate(r, fns, calls, warmup, rounds, out):
    """--rounds rounds of the calls of fns in turn: per call the median device ms over the rounds, every round, the host ms."""
    ms, host_ms = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            d, h = device_ms(r, fn, calls, warmup)
            ms[k].append(d)
            host_ms[k].append(h)
    for k in fns:
        out[k + "_ms"] = round(float(np.median(ms[k])), 4)
        out[k + "_ms_rounds"] = [round(x, 4) for x in ms[k]]
        out[k + "_host_ms"] = round(float(np.median(host_ms[k])), 4)


def run_morph(name, calls, warmup, rounds, dense, sparse, fraction, active):
    import morph_ref as mr
    import skin_ref as sk
    model, r = make_renderer(name)
    st0 = r.stats()
    nt = dense + sparse
    morphs = {k: mr.bumps(m.vertex, dense, sparse, fraction) for k, m in enumerate(model.meshes)}
    w = np.zeros(nt, np.float32)
    on = np.unique(np.round(np.linspace(0, nt - 1, min(active, nt))).astype(np.int64))       # spread over the dense and the sparse ones
    w[on] = np.random.default_rng(5).uniform(0.2, 1.0, len(on)).astype(np.float32)
    weights = {k: w.copy() for k in morphs}
    t = time.perf_counter()
    r.set_morphs(morphs)
    set_morphs_ms = (time.perf_counter() - t) * 1e3
    host = mr.restate(model, morphs, weights)
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    torch.cuda.synchronize()
    vertices = int(sum(m.vertex.shape[0] for m in model.meshes))
    entries = int(sum(len(mr.split(t_, model.meshes[k].vertex.shape[0])[0]) for k, ts in morphs.items() for t_ in ts))
    out = dict(scene=name, triangles=model.num_triangles, meshes=len(model.meshes), bvh_nodes=int(st0.num_bvh_nodes), vertices=vertices,
               targets_dense=dense, targets_sparse=sparse, sparse_fraction=fraction, targets_active=int((w != 0).sum()),
               active_dense=int((w[:dense] != 0).sum()), entries=entries, entries_per_vertex=round(entries / max(1, vertices), 2),
               rounds=rounds, calls=calls, set_morphs_host_ms=round(set_morphs_ms, 3))
    alternate(r, dict(update_morphed=lambda: r.update_morphed(weights), update_vertices_device=lambda: r.update_vertices(dev),
                      update_vertices_host=lambda: r.update_vertices(host)), calls, warmup, rounds, out)
    p, n = C.c_void_p(), C.c_size_t()
    r._check(r._L.fovpt_debug_buffer(r._ctx, b"scene_vertices", C.byref(p), C.byref(n)))
    want = np.concatenate([host[k] for k in range(len(model.meshes))]).view(np.uint32).reshape(-1)
    r.update_morphed(weights)
    out["positions_match_restatement"] = bool(np.array_equal(r.download(p.value, np.empty(n.value // 4, np.uint32)), want))
    # morph and skin in one pass against the skin alone
    skins = {k: sk.bend(m.vertex, 2 + (7 * k) % 63) for k, m in enumerate(model.meshes)}
    pal = {k: sk.bend_pose(m.vertex, skins[k][2], 12.0, (0.0, 0.02 * (k % 5), 0.0)) for k, m in enumerate(model.meshes)}
    r.set_skins(skins)
    both = {k: (weights[k], pal[k]) for k in morphs}
    alternate(r, dict(update_morphed_skinned=lambda: r.update_morphed(both), update_skinned=lambda: r.update_skinned(pal)), calls, warmup, rounds, out)
    want = mr.restate(model, morphs, both, skins)
    want = np.concatenate([want[k] for k in range(len(model.meshes))]).view(np.uint32).reshape(-1)
    r.update_morphed(both)
    out["skinned_positions_match_restatement"] = bool(np.array_equal(r.download(p.value, np.empty(n.value // 4, np.uint32)), want))
    r.close()
    print(json.dumps(out), flush=True)


def run_rig(name, calls, warmup, rounds):
    """--rig: see the module docstring."""
    import rig_ref as rg
    import skin_ref as sk
    from oracle import oracle_py as orc
    orc.build()
    orc.set_math_mode(True)
    model, r = make_renderer(name)
    st0 = r.stats()
    rng = np.random.default_rng(11)
    n = rg.MAX_NODES
    rig = rg.random_rig(rng, n, max_depth=8, scales=False, clip_channels=0.0)
    for i in range(n):                                                    # a rotation channel of four keys on every node: small turns
        rig["translation"][i] *= np.float32(0.02)
        base = rig["rotation"][i].astype(np.float64)
        keys = [base]
        for _ in range(3):
            x1, y1, z1, w1 = keys[-1]
            x2, y2, z2, w2 = rg.quat(rng.standard_normal(3), 3.0).astype(np.float64)
            keys.append(np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                                  w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2]))
        rig["clips"][0].append(rg.channel(i, rg.ROTATION, [0.0, 1.0, 2.0, 3.0], np.stack(keys)))
    skins = {k: sk.bend(m.vertex, 2 + (7 * k) % 63) for k, m in enumerate(model.meshes)}
    for k in skins:
        nodes = ((37 * k + np.arange(skins[k][2])) % n).astype(np.uint16)
        rig["bindings"].append(dict(mesh=k, joint_nodes=nodes, inverse_bind=rg.inverse_bind_of(rig, nodes)))
    r.set_skins(skins)
    t = time.perf_counter()
    r.set_rig(rig)
    set_rig_ms = (time.perf_counter() - t) * 1e3
    T = 1.4
    pals = dict(zip(sorted(skins), rg.pose(orc, rig, 0, T)["palettes"]))   # the host's animation system, beforehand
    host = sk.restate(model, skins, pals)
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    torch.cuda.synchronize()
    out = dict(scene=name, triangles=model.num_triangles, meshes=len(model.meshes), bvh_nodes=int(st0.num_bvh_nodes),
               vertices=int(sum(m.vertex.shape[0] for m in model.meshes)), joints=int(sum(s[2] for s in skins.values())),
               rig_nodes=n, rig_levels=int(max(_levels(rig["parent"]))), rounds=rounds, calls=calls, set_rig_host_ms=round(set_rig_ms, 3))
    alternate(r, dict(update_animated=lambda: r.update_animated(0, T), update_skinned=lambda: r.update_skinned(pals),
                      update_vertices_device=lambda: r.update_vertices(dev)), calls, warmup, rounds, out)
    p, nb = C.c_void_p(), C.c_size_t()
    r._check(r._L.fovpt_debug_buffer(r._ctx, b"scene_vertices", C.byref(p), C.byref(nb)))
    r.update_animated(0, T)
    got = r.download(p.value, np.empty(nb.value // 4, np.uint32))
    out["positions_match_restatement"] = bool(np.array_equal(got, np.concatenate([host[k] for k in range(len(model.meshes))]).view(np.uint32).reshape(-1)))
    r.close()
    print(json.dumps(out), flush=True)
    # k_rig_pose by itself: a scene of a few vertices, one joint; what update_animated takes beyond update_skinned with a device
    # palette (the same launches but for k_rig_pose) on the same context, in turn
    small = scenes.cornell_box()
    for nodes in (64, 1024):
        for shape, make in (("flat", rg.flat_rig), ("chain", rg.chain_rig)):
            q = renderer.SampleRenderer(small)
            q.set_skins({4: sk.bend(small.meshes[4].vertex, 1)})
            g = make(nodes)
            g["bindings"] = [dict(mesh=4, joint_nodes=np.array([nodes - 1], np.uint16), inverse_bind=np.eye(3, 4, dtype=np.float32)[None])]
            q.set_rig(g)
            pal = {4: torch.from_numpy(np.eye(3, 4, dtype=np.float32)[None].copy()).cuda()}
            torch.cuda.synchronize()
            o = dict(scene="cornell", rig_nodes=nodes, rig_shape=shape, rig_levels=1 if shape == "flat" else nodes, rounds=rounds, calls=calls)
            alternate(q, dict(update_animated=lambda: q.update_animated(0, 0.625), update_skinned_device=lambda: q.update_skinned(pal)), calls, warmup, rounds, o)
            o["k_rig_pose_ms"] = round(o["update_animated_ms"] - o["update_skinned_device_ms"], 4)
            q.close()
            print(json.dumps(o), flush=True)


def run_async(name, frames, rounds, threshold):
    """--async: see the module docstring."""
    model, r = make_renderer(name)
    cfg = r.config
    cfg.frames_in_flight = 2
    r.config = cfg
    st0 = r.stats()
    moving = list(range(0, len(model.meshes), 4))
    identity = {k: np.eye(3, 4, dtype=np.float32) for k in range(len(model.meshes))}
    poses = [{k: turn_matrix(model.meshes[k].vertex, 3.0 * (f + 1)) for k in moving} for f in range(frames)]
    stream = torch.cuda.ExternalStream(r.stream)
    r.hierarchy_cost()                                          # watching: the caller decides on current / built
    out = dict(scene=name, triangles=model.num_triangles, meshes=len(model.meshes), moving_meshes=len(moving), frames=frames, rounds=rounds,
               threshold=threshold, build_ms_set_scene=round(st0.ms_bvh_build, 3))

    def timed(calls, key, fn, building):
        t = time.perf_counter()
        v = fn()
        calls.append((key, (time.perf_counter() - t) * 1e3, building))
        return v

    def loop(mode):
        r.update_transforms(identity, rebuild=True)             # from rest, on a fresh tree, the device idle
        r.synchronize()
        calls, marks, building_frames, adopt_frames, rebuilds = [], [], [], [], 0
        request_t, ready_ms, build_ms = None, [], []
        want, adopted = False, 0
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(frames + 1)]
        ev[0].record(stream)
        for f in range(frames):
            if f >= 2:
                ev[f - 1].synchronize()                         # two frames in flight, as an application's present would hold it: frame f - 2 is done
            building = False
            if mode == "async":
                s = timed(calls, "rebuild_state", r.rebuild_state, request_t is not None)
                building = s.state == abi.REBUILD_BUILDING
                if request_t is not None and s.state != abi.REBUILD_BUILDING:
                    ready_ms.append((time.perf_counter() - request_t) * 1e3)
                    build_ms.append(s.ms_build)
                    request_t = None
                if s.adopted != adopted:
                    adopted = s.adopted
                    adopt_frames.append(f - 1)                  # the previous frame's update adopted
                ask = want and s.state == abi.REBUILD_IDLE
                flag = "async" if ask else False
            else:
                ask = want
                flag = bool(want)
            timed(calls, "update_rebuild" if (ask and mode == "sync") else "update", lambda: r.update_transforms(poses[f], rebuild=flag), building)
            if ask:
                want, rebuilds = False, rebuilds + 1
                if mode == "async":
                    request_t, building = time.perf_counter(), True
            r.launchParams.frame.subframe_index = 0
            timed(calls, "render", r.render_async, building)
            c = timed(calls, "hierarchy_cost", r.hierarchy_cost, building)
            if c.built > 0 and c.current / c.built > threshold and request_t is None:
                want = True
            ev[f + 1].record(stream)
            marks.append(building)
        late = None
        if mode == "async":
            if request_t is not None:                           # still BUILDING behind the last frame: how long the request has taken once it is READY
                t_issued = time.perf_counter()
                s = r.rebuild_state(wait=True)
                late = dict(request_to_ready_ms=round((time.perf_counter() - request_t) * 1e3, 3),
                            of_which_after_the_last_frame_was_issued_ms=round((time.perf_counter() - t_issued) * 1e3, 3),
                            build_device_ms=round(s.ms_build, 3), state=int(s.state))
            else:
                r.rebuild_state(wait=True)
        r.synchronize()
        iv = np.array([ev[k].elapsed_time(ev[k + 1]) for k in range(frames)])
        marks = np.array(marks)
        res = dict(rebuilds=rebuilds, interval_mean_ms=round(float(iv.mean()), 4), interval_max_ms=round(float(iv.max()), 4),
                   interval_median_ms=round(float(np.median(iv)), 4), total_ms=round(float(iv.sum()), 3))
        for key in sorted(set(k for k, _, _ in calls)):
            res["host_max_ms_" + key] = round(max(t for k, t, _ in calls if k == key), 4)
            res["host_median_ms_" + key] = round(float(np.median([t for k, t, _ in calls if k == key])), 4)
        if mode == "async":
            during = [t for k, t, b in calls if b]
            res["host_max_ms_any_call_while_building"] = round(max(during), 4) if during else None
            res["request_to_ready_ms"] = [round(x, 3) for x in ready_ms]
            res["build_device_ms"] = [round(x, 3) for x in build_ms]
            res["frames_while_building"] = int(marks.sum())
            res["interval_mean_ms_while_building"] = round(float(iv[marks].mean()), 4) if marks.any() else None
            res["interval_mean_ms_otherwise"] = round(float(iv[~marks].mean()), 4) if (~marks).any() else None
            res["interval_ms_of_adopting_frames"] = [round(float(iv[k]), 4) for k in adopt_frames if 0 <= k < frames]
            res["adopted"] = int(adopted)
            res["ready_only_after_the_loop"] = late
        return res

    out["loops"] = []
    for k in range(rounds):
        for mode in ("sync", "async"):
            res = loop(mode)
            res["mode"], res["round"] = mode, k
            out["loops"].append(res)
    # the device time of an adoption alone: an idle device, a finished build, events around rebuild_state(adopt)
    r.update_transforms(identity, rebuild=True)
    r.update_transforms({}, rebuild="async")
    r.rebuild_state(wait=True)
    r.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    t = time.perf_counter()
    r.rebuild_state(adopt=True)
    out["adopt_host_ms"] = round((time.perf_counter() - t) * 1e3, 4)
    b.record(stream)
    b.synchronize()
    out["adopt_device_ms"] = round(a.elapsed_time(b), 4)
    t = time.perf_counter()
    r.rebuild_state()                                           # the poll that releases the retired hierarchy (hipFree)
    out["release_poll_host_ms"] = round((time.perf_counter() - t) * 1e3, 4)
    r.close()
    print(json.dumps(out), flush=True)


def _levels(parent):
    lv = []
    for p in parent:
        lv.append(1 if p < 0 else lv[int(p)] + 1)
    return lv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c3,street")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--transforms", action="store_true", help="fovpt_update_transforms and fovpt_hierarchy_cost instead of fovpt_update_vertices")
    ap.add_argument("--skin", action="store_true", help="fovpt_update_skinned against fovpt_update_vertices with device pointers and with host arrays")
    ap.add_argument("--morph", action="store_true", help="fovpt_update_morphed against fovpt_update_vertices with device pointers and with host arrays, and with matrices against fovpt_update_skinned")
    ap.add_argument("--rig", action="store_true", help="fovpt_update_animated against fovpt_update_skinned with host palettes and fovpt_update_vertices with device pointers, and k_rig_pose by itself")
    ap.add_argument("--async", dest="async_", action="store_true", help="FOVPT_UPDATE_REBUILD_ASYNC against FOVPT_UPDATE_REBUILD in a frame loop with large motion")
    ap.add_argument("--threshold", type=float, default=2.0, help="--async: a rebuild is asked for when current / built exceeds it")
    ap.add_argument("--morph-dense", type=int, default=8)
    ap.add_argument("--morph-sparse", type=int, default=44)
    ap.add_argument("--morph-fraction", type=float, default=0.05)
    ap.add_argument("--morph-active", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5, help="--transforms, --skin, --morph, --rig: rounds of the alternated timings (at least 5)")
    a = ap.parse_args()
    for s in a.scenes.split(","):
        if a.async_:
            run_async(s, a.frames, a.rounds, a.threshold)
        elif a.rig:
            run_rig(s, a.calls, a.warmup, max(5, a.rounds))
        elif a.morph:
            run_morph(s, a.calls, a.warmup, max(5, a.rounds), a.morph_dense, a.morph_sparse, a.morph_fraction, a.morph_active)
        elif a.skin:
            run_skin(s, a.calls, a.warmup, max(5, a.rounds))
        elif a.transforms:
            run_transforms(s, a.calls, a.warmup, a.frames, max(5, a.rounds))
        else:
            run(s, a.calls, a.warmup, a.frames)


if __name__ == "__main__":
    main()
