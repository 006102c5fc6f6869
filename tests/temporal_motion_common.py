"""Checks of fovpt_temporal_motion on the GPU against tests/temporal_motion_ref.py (MotionChecker, restate and the ramp's
geometry): used by the tests of the stages that move meshes.  General helpers are in tests/gpu_common.py.

Like temporal_common.Checker, every expectation is computed from the GPU's own inputs: the input frame, the G-buffer and hit
records fovpt_gbuffer builds at the current camera after the step (it traces the same rays), the G-buffer and history of the
previous step, and the vertex arrays the test itself uploaded."""
import numpy as np

import morph_ref as mr
import skin_ref as sk
import temporal_motion_ref as tm
import temporal_ref as tr
import transform_ref as tf

from gpu_common import bits, camera, debug_buffer
from temporal_common import cap_map, tcfg

KINDS = ("vertices", "transforms", "skinned", "morphed")
METHODS = dict(vertices="update_vertices", transforms="update_transforms", skinned="update_skinned", morphed="update_morphed")


def vertex_arrays(model):
    """(tri_vidx (T, 3), vtx (V, 3), mesh_of_prim (T,), first vertex per mesh (meshes + 1,)) of a model."""
    base, vidx, vtx, mesh_of, first = 0, [], [], [], [0]
    for k, m in enumerate(model.meshes):
        vidx.append(np.asarray(m.index, np.int64) + base)
        vtx.append(np.asarray(m.vertex, np.float32))
        mesh_of.append(np.full(m.index.shape[0], k, np.int64))
        base += m.vertex.shape[0]
        first.append(base)
    return np.concatenate(vidx), np.concatenate(vtx), np.concatenate(mesh_of), np.array(first)


def download_hits(r):
    """The hit records of the last G-buffer trace: (H, W, 4) float32 (t, u, v, record offset bits)."""
    f = r.launchParams.frame
    p, n = debug_buffer(r, "gbuffer_hit")
    assert n == f.size.x * f.size.y * 16
    return r.download(p, np.empty((f.size.y, f.size.x, 4), np.float32))


def restate(model, kind, updates, skins=None, morphs=None):
    """One update of `kind` (KINDS) restated -> (what the renderer's method of that kind is given, {mesh: new positions}).
    updates maps a mesh to its vertices, its matrix, its palette, or its weights / (weights, palette); the new positions are
    transform_ref's, skin_ref's and morph_ref's over the model's rest positions and the registered skins and morphs."""
    if kind == "vertices":
        give = ups = {k: np.ascontiguousarray(v, np.float32) for k, v in updates.items()}
    elif kind == "transforms":
        give = {k: tf.matrix(m) for k, m in updates.items()}
        ups = tf.restate(model, give)
    elif kind == "skinned":
        give = {k: np.ascontiguousarray(sk.palette(p).reshape(-1, 3, 4)) for k, p in updates.items()}
        ups = sk.restate(model, skins, give)
    else:
        assert kind == "morphed", kind
        give = {k: ((np.ascontiguousarray(p[0], np.float32), np.ascontiguousarray(sk.palette(p[1]).reshape(-1, 3, 4))) if isinstance(p, tuple)
                    else np.ascontiguousarray(p, np.float32)) for k, p in updates.items()}
        ups = mr.restate(model, morphs, give, skins)
    return give, ups


class MotionChecker:
    """Follows one renderer's updates and temporal steps.  update() moves meshes and remembers it; step() runs
    fovpt_temporal_motion (or, plain=True, fovpt_temporal) and compares colour, rgba8, history and motion vectors with the
    restatement, given the meshes moved since the previous step and the positions all vertices had when it ran.  It follows the
    tracking rule too: made for a context that has not stepped with motion yet (a new one, or after fovpt_set_scene), it expects
    no history of a fovpt_temporal_motion step when an update ran since the previous step before the first such step."""

    def __init__(self, oracle, r, d=None):
        self.oracle, self.r, self.d = oracle, r, dict(d or {})
        self.tri_vidx, self.vtx, self.mesh_of_prim, self.first = vertex_arrays(r.model)
        self.vtx = self.vtx.copy()
        self.vtx_step = self.vtx.copy()                     # the positions when the previous step ran
        self.moved = np.zeros(len(r.model.meshes), bool)
        self.prev = None
        self.tracking = self.untracked = False
        self._keep = None
        self.skins, self.morphs = {}, {}                    # what update(kind="skinned" / "morphed") restates over

    def reset(self):
        self.prev = None

    def update(self, updates, rebuild=False, device=False, kind="vertices"):
        """Moves meshes through the entry point of `kind` (KINDS): updates maps a mesh to what the renderer's method of that kind
        takes for it.  The positions the checker goes on with are restate()'s over self.skins / self.morphs, which the caller
        keeps equal to what it registered.  device: as CUDA tensors (not for transforms, which have no such form)."""
        give, ups = restate(self.r.model, kind, updates, self.skins, self.morphs)
        if device:
            import torch
            assert kind != "transforms"

            def dev(x):
                return tuple(dev(y) for y in x) if isinstance(x, tuple) else torch.from_numpy(x).cuda()
            self._keep = give = {k: dev(v) for k, v in give.items()}
            torch.cuda.synchronize()
        getattr(self.r, METHODS[kind])(give, rebuild=rebuild)
        for k, v in ups.items():
            self.vtx[self.first[k]:self.first[k + 1]] = v
            self.moved[k] = True
        self.untracked = self.untracked or (bool(ups) and not self.tracking)

    def motion(self):
        return dict(tri_vidx=self.tri_vidx, vtx_prev=self.vtx_step, vtx=self.vtx, mesh_of_prim=self.mesh_of_prim, moved=self.moved.copy())

    def step(self, inp=None, in_ptr=None, plain=False, with_motion=True):
        """-> (colour, history, cap, motion vectors or None)"""
        r = self.r
        inp = r.downloadAccum() if inp is None else inp
        if plain:
            r.temporal(tcfg(self.d), in_ptr)
        else:
            r.temporal_motion(tcfg(self.d), in_ptr, None, None, r.motion_buffer() if with_motion else None)
        f = r.launchParams.frame
        shape = (f.size.y, f.size.x)
        got_c, got_px, got_h = r.downloadTemporalColor(), r.downloadTemporalPixels(), r.downloadTemporalHistory()
        got_m = r.downloadMotion() if with_motion and not plain else None
        gb = r.downloadGBuffer()
        uv = download_hits(r)[..., 1:3]
        cam, cap = camera(r), cap_map(r, self.d)
        if not plain:
            if self.untracked:
                self.prev = None
            self.tracking = True
        self.untracked = False
        want_c, want_h, want_m = tm.step(inp, gb, uv, cap, cam, self.prev, self.d, None if plain else self.motion())
        assert np.array_equal(bits(got_c), bits(want_c))
        assert np.array_equal(bits(got_h), bits(want_h))
        assert np.array_equal(got_px, self.oracle.make_color(want_c[..., :3].reshape(-1, 3)).reshape(shape))
        if got_m is not None:
            assert np.array_equal(bits(got_m), bits(want_m))
        self.prev = dict(gb=gb, cam=cam, history=got_h)
        self.vtx_step = self.vtx.copy()
        self.moved[:] = False
        return got_c, got_h, cap, got_m


# ---- the independent geometry check ("ramp") ------------------------------------------------------------------------------
def project64(X, cam, size):
    """Pixel coordinates (pixel centres at integers, as the step's px, py) of the points X (..., 3) in cam, in binary64."""
    A = np.stack([np.array(cam[k], np.float64) for k in ("U", "V", "W")], axis=1)
    v = np.asarray(X, np.float64) - np.array(cam["eye"], np.float64)
    a = np.linalg.solve(A, v.reshape(-1, 3).T).T.reshape(v.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        px = (a[..., 0] / a[..., 2] + 1) * 0.5 * size[0] - 0.5
        py = (a[..., 1] / a[..., 2] + 1) * 0.5 * size[1] - 0.5
    return px, py, a[..., 2] > 0


def near_edge(g, mesh_of_prim, margin=2):
    """Within `margin` px of a silhouette or crease of the G-buffer g: a change of mesh (or to the sky) or of face (normal)."""
    p = g["prim"]
    n = np.round(g["normal"][..., :3] * 2).astype(np.int64) + 2
    mesh = np.asarray(mesh_of_prim)[np.where(p == tr.MISS, 0, p).astype(np.int64)]
    cls = np.where(p == tr.MISS, 0, 1 + mesh * 1000 + n[..., 0] * 25 + n[..., 1] * 5 + n[..., 2])
    e = np.zeros(p.shape, bool)
    for dy in range(-margin, margin + 1):
        for dx in range(-margin, margin + 1):
            e |= np.roll(np.roll(cls, dy, 0), dx, 1) != cls
    e[:margin], e[-margin:], e[:, :margin], e[:, -margin:] = True, True, True, True
    return e


def ramp_selection(gb, uv, pg, prev_cam, size, mesh, tri_vidx, vtx_prev, mesh_of_prim):
    """The pixels the ramp test checks and where they were -> (mask (H, W), px, py (H, W) binary64): hits of `mesh` on a side
    face (|N.y| < 0.5), more than 2 px from any silhouette or crease in the current view and, at their previous place, in
    the previous view, with all four bilinear taps inside the frame.  (px, py): the binary64 projection into prev_cam of the
    binary64 barycentric point over the previous vertices."""
    prim = gb["prim"]
    hit = prim != tr.MISS
    p = np.where(hit, prim, 0).astype(np.int64)
    iv = np.asarray(tri_vidx)[p]
    vp = np.asarray(vtx_prev, np.float64)
    u, v = uv[..., 0].astype(np.float64)[..., None], uv[..., 1].astype(np.float64)[..., None]
    X = (1.0 - u - v) * vp[iv[..., 0]] + u * vp[iv[..., 1]] + v * vp[iv[..., 2]]
    px, py, front = project64(X, prev_cam, size)
    inside = front & (px >= 0) & (px < size[0] - 1) & (py >= 0) & (py < size[1] - 1)
    qx, qy = np.where(inside, np.round(px), 0).astype(np.int64), np.where(inside, np.round(py), 0).astype(np.int64)
    side = hit & (np.asarray(mesh_of_prim)[p] == mesh) & (np.abs(gb["normal"][..., 1]) < 0.5)
    mask = side & inside & ~near_edge(gb, mesh_of_prim) & ~near_edge(pg, mesh_of_prim)[qy, qx]
    return mask, px, py
