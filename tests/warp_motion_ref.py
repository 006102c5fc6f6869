"""numpy float32 restatement of fovpt_warp_motion (csrc/warp.hip, k_warp_scatter_motion): the definition the GPU kernel matches
bit for bit.

It is warp_ref.warp -- unchanged -- on a G-buffer in which every hit pixel of a mesh that moved in the interval the last temporal
step ended has its point replaced by where the surface will be `advance` intervals past the rendered frame.  With (u, v) the
pixel's hit record, P its primitive, a', b', c' the positions P's vertices had when the step before the last one ran, in the order
of the mesh's index triple, X_s the G-buffer position as stored, each line one binary32 operation per component:

    w0   (1 - u) - v
    X'   (w0 a' + u b') + v c'
    d    X_s - X'
    X*   X_s + advance * d

Pixels of unmoved meshes and misses keep the G-buffer's bits; so does every pixel when advance is 0 or no mesh moved (the library
then runs fovpt_warp's own scatter).  A non-finite X* fails warp_ref.landing's float comparisons and lands nowhere."""
import numpy as np

import warp_ref as wr

f32 = np.float32
DEFAULTS = dict(images=3, fill_radius=2, advance=1.0)
MAX_ADVANCE = 4.0


def moved_pixels(gb, motion):
    """(h, w) bool: the hit pixels on meshes that motion["moved"] marks."""
    prim = gb["prim"]
    hit = prim != wr.MISS
    p = np.where(hit, prim, 0).astype(np.int64)
    return hit & np.asarray(motion["moved"], bool)[np.asarray(motion["mesh_of_prim"], np.int64)[p]]


def extrapolate(gb, uv, motion, advance):
    """-> the G-buffer with position.xyz of the moved meshes' hit pixels replaced by X*.

    motion: the dict MotionChecker.motion() produces for the interval -- tri_vidx (T, 3) vertex indices per global primitive id,
    vtx_prev (V, 3) float32 the positions when the interval began, mesh_of_prim (T,), moved (meshes,) bool."""
    advance = f32(advance)
    sel = moved_pixels(gb, motion)
    if advance == 0 or not sel.any():
        return gb
    iv = np.asarray(motion["tri_vidx"], np.int64)[gb["prim"][sel].astype(np.int64)]
    prev = np.asarray(motion["vtx_prev"], np.float32)
    A, B, C = prev[iv[:, 0]], prev[iv[:, 1]], prev[iv[:, 2]]
    u, v = np.ascontiguousarray(uv[..., 0], np.float32)[sel][:, None], np.ascontiguousarray(uv[..., 1], np.float32)[sel][:, None]
    Xs = np.ascontiguousarray(gb["position"][..., :3], np.float32)[sel]
    with np.errstate(invalid="ignore", over="ignore"):
        w0 = (f32(1.0) - u) - v
        Xp = (w0 * A + u * B) + v * C
        d = Xs - Xp
        X = Xs + advance * d
    assert X.dtype == np.float32
    out = dict(gb)
    out["position"] = gb["position"].copy()
    out["position"][sel, :3] = X
    return out


def warp(gb, uv, motion, cam, to, cfg=None, in_color=None, in_rgba=None):
    """fovpt_warp_motion -> warp_ref.warp's dict.  motion None: the last step knew of no motion."""
    cfg = dict(DEFAULTS, **(cfg or {}))
    g2 = gb if motion is None else extrapolate(gb, uv, motion, cfg["advance"])
    return wr.warp(g2, cam, to, dict(images=cfg["images"], fill_radius=cfg["fill_radius"]), in_color, in_rgba)
