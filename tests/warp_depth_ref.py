"""numpy restatement of fovpt_warp_depth (csrc/warp.hip, k_warp_scatter_depth): fovpt_warp with the source point rebuilt from a
depth image and the camera it was rendered with, ending in warp_ref's key and resolve.  Every float operation is one binary32
operation in the kernel's order.  w, h: the image size; s = y * w + x a source pixel, z = depth[s]:

    z == +inf           a miss: v = (dx U + dy V) + W of `from` (temporal_ref.miss_dirs), depth word 0x7fffffff
    0 < z < +inf        r = (dx U + dy V) + W of `from`; X_k = eye_from_k + z * r_k; v = X - eye_to
    anything else       (NaN, <= 0, -inf) the pixel scatters nothing
    then warp_ref's     a_k, px, py, fx, fy, landing test, key, scatter, resolve, outputs and counts"""
import numpy as np

import temporal_ref as tr
import warp_ref as wr

f32 = np.float32


def landing(depth, frm, to):
    """-> (dest (h, w) int64, -1 where the pixel does not land or scatters nothing; depth word (h, w) uint32)."""
    depth = np.ascontiguousarray(depth, np.float32)
    h, w = depth.shape
    M = tr.camera_inverse(to["U"], to["V"], to["W"])
    assert M is not None and tr.camera_inverse(frm["U"], frm["V"], frm["W"]) is not None
    with np.errstate(all="ignore"):
        live = depth > 0                                                   # (NaN fails)
        miss = live & np.isinf(depth)
        r = tr.miss_dirs(w, h, frm["U"], frm["V"], frm["W"]).astype(np.float32)
        z = np.where(live & ~miss, depth, f32(1.0))[..., None]
        X = np.asarray(frm["eye"], np.float32) + z * r
        v = np.where(miss[..., None], r, X - np.asarray(to["eye"], np.float32)).astype(np.float32)
        a = [(M[k, 0] * v[..., 0] + M[k, 1] * v[..., 1]) + M[k, 2] * v[..., 2] for k in range(3)]
        fw, fh = f32(w), f32(h)
        px = (((a[0] / a[2]) + f32(1.0)) * f32(0.5)) * fw - f32(0.5)
        py = (((a[1] / a[2]) + f32(1.0)) * f32(0.5)) * fh - f32(0.5)
        fx, fy = np.floor(px + f32(0.5)), np.floor(py + f32(0.5))
        ok = live & (a[2] > 0) & (fx >= 0) & (fx < fw) & (fy >= 0) & (fy < fh)
        assert all(t.dtype == np.float32 for t in (X, px, py, fx, fy))
    ix, iy = np.where(ok, fx, 0).astype(np.int64), np.where(ok, fy, 0).astype(np.int64)
    dest = np.where(ok, iy * w + ix, -1)
    word = np.where(miss, wr.MISS_DEPTH, np.ascontiguousarray(a[2], np.float32).view(np.uint32)).astype(np.uint32)
    return dest, word, px, py


def warp(depth, frm, to, cfg=None, in_color=None, in_rgba=None):
    """fovpt_warp_depth -> warp_ref.warp's dict, with px and py (h, w) float32 beside it."""
    cfg = dict(wr.DEFAULTS, **(cfg or {}))
    dest, word, px, py = landing(depth, frm, to)
    keys = wr.scatter(dest, word)
    src, cls = wr.resolve(keys, cfg["fill_radius"])
    flat = src.reshape(-1).astype(np.int64)
    h, w = src.shape
    out = dict(map=(src | (cls << np.uint32(30))).astype(np.uint32), keys=keys, dest=dest, depth=word, px=px, py=py, color=None, rgba=None)
    if cfg["images"] & wr.COLOR:
        out["color"] = np.ascontiguousarray(in_color, np.float32).reshape(h * w, 4)[flat].reshape(h, w, 4)
    if cfg["images"] & wr.RGBA:
        out["rgba"] = np.ascontiguousarray(in_rgba, np.uint32).reshape(h * w)[flat].reshape(h, w)
    out["counts"] = (int((dest >= 0).sum()), int((cls == wr.DIRECT).sum()), int((cls == wr.FILLED).sum()), int((cls == wr.EMPTY).sum()))
    return out
