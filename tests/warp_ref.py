"""numpy restatement of fovpt_warp (csrc/warp.hip): the definition the GPU kernels match bit for bit.

Every float operation below is one IEEE binary32 operation in the order the kernel performs it (the library is built with
-ffp-contract=off, so the device does not fuse any of them either); the `to` camera's inverse is binary64 on the host, each
entry rounded to binary32 (temporal_ref.camera_inverse).  w, h: the frame size; s = y * w + x a source pixel.

    scatter, per source pixel s
    v       hit (prim != 0xffffffff): X_s - eye_to; miss: (dx U + dy V) + W of the RENDERED camera, the G-buffer ray of the pixel
            before normalising (temporal_ref.miss_dirs): the sky is at infinity, so only rotation moves it
    a_k     (M_k.x v.x + M_k.y v.y) + M_k.z v.z, M the rows of [U V W]^-1 of `to`
    p       px = (((a.x / a.z) + 1) * 0.5) * w - 0.5 (py likewise with h); fx = floor(px + 0.5), fy likewise
    lands   a.z > 0 and 0 <= fx < w and 0 <= fy < h, compared in float (NaN fails)
    key     d = the bits of a.z for a hit, 0x7fffffff for a miss; key = d << 32 | s;
            keys[fy * w + fx] = min(keys[...], key), keys all ones before: the nearest depth wins, equal depths go to the lower
            source index, whatever the order

    resolve, per destination pixel q
    direct  key not empty: class 0, src = the key's low word
    filled  key empty: for r = 1 .. fill_radius the pixels at Chebyshev distance exactly r inside the frame; the first r with a
            non-empty key ends the search: class 1, src = the low word of the LARGEST key of that ring
    empty   still none: class 2, src = q
    out     out_color[q] = in_color[src] (all four components, bit for bit), out_rgba[q] = in_rgba[src],
            out_map[q] = src | class << 30

    counts  splatted: the source pixels that land; direct, filled, empty: the destination pixels by class"""
import numpy as np

import temporal_ref as tr

f32 = np.float32
DEFAULTS = dict(images=3, fill_radius=2)
COLOR, RGBA = 1, 2
MAX_RADIUS = 4
DIRECT, FILLED, EMPTY = 0, 1, 2
MISS = np.uint32(0xffffffff)
NO_KEY = np.uint64(0xffffffffffffffff)
MISS_DEPTH = np.uint32(0x7fffffff)


def landing(gb, cam, to):
    """-> (dest (h, w) int64: fy * w + fx where the source pixel lands, -1 where it does not; depth (h, w) uint32: its depth
    word).  gb: dict prim (h, w) uint32, position (h, w, 4) float32; cam: the rendered camera, to: the camera warped to, dicts
    of eye / U / V / W.  A singular `to` is refused by the library: None here."""
    h, w = gb["prim"].shape
    M = tr.camera_inverse(to["U"], to["V"], to["W"])
    if M is None:
        return None
    miss = gb["prim"] == MISS
    X = np.ascontiguousarray(gb["position"][..., :3], np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.where(miss[..., None], tr.miss_dirs(w, h, cam["U"], cam["V"], cam["W"]), X - np.asarray(to["eye"], np.float32)).astype(np.float32)
        a = [(M[k, 0] * v[..., 0] + M[k, 1] * v[..., 1]) + M[k, 2] * v[..., 2] for k in range(3)]
    fw, fh = f32(w), f32(h)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        px = (((a[0] / a[2]) + f32(1.0)) * f32(0.5)) * fw - f32(0.5)
        py = (((a[1] / a[2]) + f32(1.0)) * f32(0.5)) * fh - f32(0.5)
        fx, fy = np.floor(px + f32(0.5)), np.floor(py + f32(0.5))
        ok = (a[2] > 0) & (fx >= 0) & (fx < fw) & (fy >= 0) & (fy < fh)
        assert all(t.dtype == np.float32 for t in (px, py, fx, fy))
    ix, iy = np.where(ok, fx, 0).astype(np.int64), np.where(ok, fy, 0).astype(np.int64)
    dest = np.where(ok, iy * w + ix, -1)
    depth = np.where(miss, MISS_DEPTH, np.ascontiguousarray(a[2], np.float32).view(np.uint32)).astype(np.uint32)
    return dest, depth


def scatter(dest, depth):
    """The keys (h, w) uint64 of the landing."""
    h, w = dest.shape
    s = np.arange(h * w, dtype=np.uint64)
    key = (depth.reshape(-1).astype(np.uint64) << np.uint64(32)) | s
    keys = np.full(h * w, NO_KEY, np.uint64)
    on = dest.reshape(-1) >= 0
    np.minimum.at(keys, dest.reshape(-1)[on], key[on])
    return keys.reshape(h, w)


def resolve(keys, fill_radius):
    """-> (src (h, w) uint32, cls (h, w) uint32)."""
    h, w = keys.shape
    R = int(fill_radius)
    assert 0 <= R <= MAX_RADIUS
    q = np.arange(h * w, dtype=np.uint32).reshape(h, w)
    have = keys != NO_KEY
    src = np.where(have, (keys & np.uint64(0xffffffff)).astype(np.uint32), q)
    cls = np.where(have, DIRECT, EMPTY).astype(np.uint32)
    # an empty or outside pixel counts as key 0 in a ring's maximum: no landed key is 0 (a landed depth word is above 0)
    pad = np.zeros((h + 2 * R, w + 2 * R), np.uint64)
    pad[R:R + h, R:R + w] = np.where(have, keys, np.uint64(0))
    todo = ~have
    for r in range(1, R + 1):
        best = np.zeros((h, w), np.uint64)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if max(abs(dx), abs(dy)) == r:
                    best = np.maximum(best, pad[R + dy:R + dy + h, R + dx:R + dx + w])
        got = todo & (best != 0)
        src = np.where(got, (best & np.uint64(0xffffffff)).astype(np.uint32), src)
        cls = np.where(got, np.uint32(FILLED), cls)
        todo &= ~got
    return src.astype(np.uint32), cls.astype(np.uint32)


def warp(gb, cam, to, cfg=None, in_color=None, in_rgba=None):
    """fovpt_warp -> dict(color (h, w, 4) float32 or None, rgba (h, w) uint32 or None, map (h, w) uint32, counts (splatted,
    direct, filled, empty), keys, dest, depth); an image that cfg["images"] leaves out is None."""
    cfg = dict(DEFAULTS, **(cfg or {}))
    dest, depth = landing(gb, cam, to)
    keys = scatter(dest, depth)
    src, cls = resolve(keys, cfg["fill_radius"])
    flat = src.reshape(-1).astype(np.int64)
    h, w = src.shape
    out = dict(map=(src | (cls << np.uint32(30))).astype(np.uint32), keys=keys, dest=dest, depth=depth, color=None, rgba=None)
    if cfg["images"] & COLOR:
        out["color"] = np.ascontiguousarray(in_color, np.float32).reshape(h * w, 4)[flat].reshape(h, w, 4)
    if cfg["images"] & RGBA:
        out["rgba"] = np.ascontiguousarray(in_rgba, np.uint32).reshape(h * w)[flat].reshape(h, w)
    out["counts"] = (int((dest >= 0).sum()), int((cls == DIRECT).sum()), int((cls == FILLED).sum()), int((cls == EMPTY).sum()))
    return out


def collisions(dest):
    """-> (landed (h * w) int64: the number of sources that land on each destination pixel)."""
    d = dest.reshape(-1)
    return np.bincount(d[d >= 0], minlength=d.size)


def winner_is_not_lowest(dest, keys):
    """Destination pixels whose winning source is not the lowest-index source that lands there (h * w bool)."""
    d = dest.reshape(-1)
    n = d.size
    lowest = np.full(n, n, np.int64)
    on = d >= 0
    np.minimum.at(lowest, d[on], np.arange(n)[on])
    k = keys.reshape(-1)
    have = k != NO_KEY
    return have & ((k & np.uint64(0xffffffff)).astype(np.int64) != lowest)
