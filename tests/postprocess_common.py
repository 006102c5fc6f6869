"""Shared checks of the post-processing of a rendered frame (fovpt_denoise, fovpt_gbuffer, fovpt_reconstruct) against their
numpy restatements (tests/denoise_ref.py, tests/reconstruct_ref.py) and the oracle: used by test_denoise_gpu.py,
test_reconstruct_gpu.py and test_postprocess_fuzz_gpu.py.  The box scene and the other helpers no stage owns are in
tests/gpu_common.py.

Every expectation is computed from the GPU's own inputs (guide buffers, accum buffer, G-buffer) and from the frame's
description -- size, gaze, radii, FOV_OFF flag -- as the frame was rendered: by default r.launchParams and cfg, which the
callers leave as they were at render time."""
import numpy as np

import denoise_ref as dn
import reconstruct_ref as rr
from fovpathtracing_optixcodelatest_amd import abi, lib

from gpu_common import bits, with_entries


def _f32(a):
    return np.asarray(a, np.float32)


def _gaze(r, gaze):
    f = r.launchParams.frame
    return (f.c.x, f.c.y) if gaze is None else tuple(int(v) & 0xffffffff for v in gaze)


def guides(r):
    f = r.launchParams.frame
    shape = (f.size.y, f.size.x, 4)
    return [r.download(p, np.empty(shape, np.float32)) for p in (f.color_buffer, f.normal_buffer, f.albedo_buffer)]


def dcfg(d):
    """fovpt_denoise_defaults with the entries of d replaced."""
    c = abi.DenoiseConfig()
    lib.check(None, lib.load().fovpt_denoise_defaults(c))
    return with_entries(c, d)


def rcfg(d):
    """fovpt_reconstruct_defaults with the entries of d replaced."""
    c = abi.ReconstructConfig()
    lib.check(None, lib.load().fovpt_reconstruct_defaults(c))
    return with_entries(c, d)


# ---- fovpt_denoise -------------------------------------------------------------------------------------------------------
def expected_denoise(r, cfg, d=None, gaze=None):
    """The restatement over the GPU's guide buffers for the frame r rendered last with cfg (and gaze: default lp's)
    -> (colour, iterations per pixel, pass per pixel)."""
    f = r.launchParams.frame
    color, normal, albedo = guides(r)
    fill, pas = dn.level_map(f.size.x, f.size.y, _gaze(r, gaze), cfg.r_inner, cfg.r_outer, cfg.uniform)
    d = dict(dn.DEFAULTS, **(d or {}))
    n = dn.iteration_map(fill, pas, d, cfg.uniform)
    out, _ = dn.denoise(color, normal, albedo, fill, n, d)
    return out, n, pas


def check_denoise(oracle, r, cfg, d=None, gaze=None):
    """r.denoise(d) into the renderer's own buffers: colour bit for bit the restatement, rgba8 its tone map."""
    r.denoise(dcfg(d) if d else None)
    got_c, got_px = r.downloadDenoisedColor(), r.downloadDenoisedPixels()
    want, n, pas = expected_denoise(r, cfg, d, gaze)
    assert np.array_equal(bits(got_c), bits(want))
    assert np.array_equal(got_px, oracle.make_color(want[..., :3].reshape(-1, 3)).reshape(got_px.shape))
    return got_c, n, pas


# ---- fovpt_gbuffer -------------------------------------------------------------------------------------------------------
def camera_rays(r):
    """fovpt_gbuffer's rays for r's frame size and current camera."""
    f, cam = r.launchParams.frame, r.launchParams.camera
    vec = lambda v: (v.x, v.y, v.z)
    return rr.primary_rays(f.size.x, f.size.y, vec(cam.eye), vec(cam.U), vec(cam.V), vec(cam.W))


def expected_gbuffer(oracle, model, r):
    """The G-buffer restated: numpy rays, the oracle's closest hit, numpy float32 cross / normalize, oracle tex2d."""
    f = r.launchParams.frame
    w, h = f.size.x, f.size.y
    o, d = camera_rays(r)
    prim, tuv, _ = oracle.OracleScene(model).trace(o, d)
    # global primitive order: mesh order, then index order (fovpt_set_scene)
    tri = np.concatenate([_f32(m.vertex)[np.asarray(m.index, np.int64)] for m in model.meshes])          # (T, 3, 3)
    mesh_of = np.concatenate([np.full(len(m.index), k) for k, m in enumerate(model.meshes)])
    hit = prim != rr.MISS
    p = np.where(hit, prim, 0).astype(np.int64)
    t, u, v = tuv[:, 0], tuv[:, 1], tuv[:, 2]
    e1, e2 = tri[p, 1] - tri[p, 0], tri[p, 2] - tri[p, 0]
    c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    n0 = c * (np.float32(1.0) / np.sqrt(rr._dot(c, c)))[:, None]
    nrm = n0 * np.copysign(np.float32(1.0), rr._dot(-d, n0))[:, None]
    pos = o + t[:, None] * d
    alb = np.zeros((len(p), 3), np.float32)
    for k, m in enumerate(model.meshes):
        sel = hit & (mesh_of[p] == k)
        if m.texture_id >= 0 and m.texcoord is not None:
            tc = _f32(m.texcoord)[np.asarray(m.index, np.int64)]                                           # (Tm, 3, 2)
            first = int(np.flatnonzero(mesh_of == k)[0])
            q = tc[p[sel] - first]
            w0 = (np.float32(1.0) - u[sel]) - v[sel]
            uv = (w0[:, None] * q[:, 0] + u[sel][:, None] * q[:, 1]) + v[sel][:, None] * q[:, 2]
            alb[sel] = oracle.tex2d(model.textures[m.texture_id], uv)[:, :3]
        else:
            alb[sel] = np.float32([m.material.color.x, m.material.color.y, m.material.color.z])
    out = dict(prim=prim.reshape(h, w), position=np.zeros((h * w, 4), np.float32), normal=np.zeros((h * w, 4), np.float32),
               albedo=np.zeros((h * w, 4), np.float32))
    out["position"][:, 3] = -1.0
    out["position"][hit] = np.concatenate([pos, t[:, None]], axis=1)[hit]
    out["normal"][hit, :3] = nrm[hit]
    out["albedo"][hit, :3] = alb[hit]
    for k in ("position", "normal", "albedo"):
        out[k] = out[k].reshape(h, w, 4)
    return out


def check_gbuffer_prim(r, gb, rows=None):
    """The G-buffer's prim is what the production traversal (fovpt_debug_trace) returns on the same rays; rows: the frame's
    rows to trace (default all)."""
    f = r.launchParams.frame
    o, d = camera_rays(r)
    ys = np.arange(f.size.y) if rows is None else np.asarray(rows)
    sel = (ys[:, None] * f.size.x + np.arange(f.size.x)[None, :]).reshape(-1)
    assert np.array_equal(r.debug_trace(o[sel], d[sel])[0].reshape(len(ys), f.size.x), gb["prim"][ys])


# ---- fovpt_reconstruct ---------------------------------------------------------------------------------------------------
def expected_reconstruct(r, cfg, d=None, in_color=None, gaze=None, gb=None):
    """The restatement over the GPU's albedo guide and G-buffer (gb, default: built now with r's camera) for the frame r
    rendered last with cfg -> (colour, fill per pixel)."""
    f = r.launchParams.frame
    shape = (f.size.y, f.size.x, 4)
    albedo = r.download(f.albedo_buffer, np.empty(shape, np.float32))
    inp = in_color if in_color is not None else r.downloadAccum()
    fill, _, ax, ay = rr.writers(f.size.x, f.size.y, _gaze(r, gaze), cfg.r_inner, cfg.r_outer, cfg.uniform)
    gb = gb if gb is not None else r.downloadGBuffer()
    return rr.reconstruct(inp, albedo, gb, fill, ax, ay, d), fill


def check_reconstruct(oracle, r, cfg, d=None, in_color=None, in_ptr=None, gaze=None):
    """r.reconstruct(d, in_ptr) into the renderer's own buffers: colour bit for bit the restatement, rgba8 its tone map."""
    r.reconstruct(rcfg(d) if d else None, in_ptr)
    got_c, got_px = r.downloadReconstructedColor(), r.downloadReconstructedPixels()
    want, fill = expected_reconstruct(r, cfg, d, in_color, gaze)
    assert np.array_equal(bits(got_c), bits(want))
    assert np.array_equal(got_px, oracle.make_color(want[..., :3].reshape(-1, 3)).reshape(got_px.shape))
    return got_c, fill
