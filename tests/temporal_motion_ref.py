"""numpy float32 restatement of fovpt_temporal_motion (csrc/temporal.hip, k_temporal_motion): the definition the GPU kernel
matches bit for bit.

It is temporal_ref.step -- unchanged -- on a G-buffer in which every hit pixel p of a moved mesh has its point and normal
replaced by where the surface was when the previous step ran.  With (u, v) the pixel's hit record, P its primitive, a', b', c'
the previous positions of P's vertices in the order of the mesh's index triple, each line one binary32 operation per component:

    w0   (1 - u) - v
    X'   (w0 a' + u b') + v c'
    N0'  normalize(cross(b' - a', c' - a')): cross = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x),
         normalize(n) = n * (1 / sqrt((n.x n.x + n.y n.y) + n.z n.z))
    s    copysign(1, dot(wo, N_0)): what k_gbuffer_fill applied to the pixel's current normal; N_0 the same normalize(cross) over
         the CURRENT positions of P's vertices, wo = -normalize((dx U + dy V) + W) the pixel's G-buffer ray reversed
    N'   N0' * s

t_p stays the current hit distance.  A degenerate previous triangle gives a non-finite N': every comparison of
temporal_ref.step fails for the pixel and it gets n = 1.  Pixels of unmoved meshes and misses keep the G-buffer's bits.

motion_out (h, w, 4): (px - x, py - y, a.z, 1) where the pixel reprojects (temporal_ref.project on the substituted G-buffer,
whatever the pixel's cap), (0, 0, 0, 0) where it does not and on a step without history."""
import numpy as np

import temporal_ref as tr

f32 = np.float32


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _normalize(v):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = f32(1.0) / np.sqrt(tr._dot(v, v))
        return v * inv[..., None]


def substitute(gb, uv, cam, motion):
    """-> the G-buffer with (position.xyz, normal.xyz) of the hit pixels of moved meshes replaced by (X', N').

    motion: dict tri_vidx (T, 3) vertex indices per global primitive id, vtx_prev / vtx (V, 3) float32 the previous and the
    current positions, mesh_of_prim (T,), moved (meshes,) bool."""
    prim = gb["prim"]
    h, w = prim.shape
    hit = prim != tr.MISS
    p = np.where(hit, prim, 0).astype(np.int64)
    sel = hit & np.asarray(motion["moved"], bool)[np.asarray(motion["mesh_of_prim"], np.int64)[p]]
    if not sel.any():
        return gb
    iv = np.asarray(motion["tri_vidx"], np.int64)[p[sel]]
    prev, cur = np.asarray(motion["vtx_prev"], np.float32), np.asarray(motion["vtx"], np.float32)
    A, B, C = prev[iv[:, 0]], prev[iv[:, 1]], prev[iv[:, 2]]
    u, v = np.ascontiguousarray(uv[..., 0], np.float32)[sel][:, None], np.ascontiguousarray(uv[..., 1], np.float32)[sel][:, None]
    w0 = (f32(1.0) - u) - v
    X = (w0 * A + u * B) + v * C
    N0p = _normalize(_cross(B - A, C - A))
    a, b, c = cur[iv[:, 0]], cur[iv[:, 1]], cur[iv[:, 2]]
    N_0 = _normalize(_cross(b - a, c - a))
    wo = -_normalize(tr.miss_dirs(w, h, cam["U"], cam["V"], cam["W"])[sel])
    with np.errstate(invalid="ignore"):
        s = np.copysign(f32(1.0), tr._dot(wo, N_0)).astype(np.float32)
        N = N0p * s[:, None]
    out = dict(gb)
    out["position"] = gb["position"].copy()
    out["normal"] = gb["normal"].copy()
    out["position"][sel, :3] = X
    out["normal"][sel, :3] = N
    return out


def step(inp, gb, uv, cap, cam, prev=None, cfg=None, motion=None):
    """One step -> (out_color, history, motion_out), each (h, w, 4) float32.  inp, gb, cap, cam, prev, cfg: as
    temporal_ref.step; uv: (h, w, 2) the hit records' (u, v) (unused without motion); motion: None, or substitute()'s dict."""
    g2 = gb if motion is None else substitute(gb, uv, cam, motion)
    out, hist = tr.step(inp, g2, cap, cam, prev, cfg)
    h, w = cap.shape
    mo = np.zeros((h, w, 4), np.float32)
    M = None
    if prev is not None and prev["history"].shape[:2] == (h, w):
        M = tr.camera_inverse(prev["cam"]["U"], prev["cam"]["V"], prev["cam"]["W"])
    if M is not None:
        px, py, ok = tr.project(g2, cam, prev["cam"], M)
        miss = g2["prim"] == tr.MISS
        X = np.ascontiguousarray(g2["position"][..., :3], np.float32)
        v = np.where(miss[..., None], tr.miss_dirs(w, h, cam["U"], cam["V"], cam["W"]), X - np.asarray(prev["cam"]["eye"], np.float32))
        az = (M[2, 0] * v[..., 0] + M[2, 1] * v[..., 1]) + M[2, 2] * v[..., 2]
        y, x = np.mgrid[0:h, 0:w]
        with np.errstate(invalid="ignore", over="ignore"):
            mo[..., 0] = np.where(ok, px - x.astype(np.float32), f32(0.0))
            mo[..., 1] = np.where(ok, py - y.astype(np.float32), f32(0.0))
            mo[..., 2] = np.where(ok, az, f32(0.0))
            mo[..., 3] = np.where(ok, f32(1.0), f32(0.0))
    return out, hist, mo
