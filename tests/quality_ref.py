"""The definition of fovpt_quality (include/fovpt.h), operation by operation, in numpy: per-class error sums, SSIM per class and the
eccentricity profile of two rgba8 images.  Everything is an integer except a window's quotient N / M, one binary64 division of two
exact integers scaled by 2^20 and rounded to an integer before it is added: no result depends on an order of summation, so the
device (csrc/quality.hip) and the host implementation (csrc/quality_host.cpp) are compared with this bit for bit.

The pixel classes come from the frame as rendered: classes_of_frame() derives them from reconstruct_ref.writers."""
import math

import numpy as np

SSIM, PROFILE = 1, 2
FOVEA, MIDDLE, PERIPHERY, UNIFORM, UNWRITTEN = range(5)
CLASSES, RINGS, MAX_RING_WIDTH = 5, 64, 65536
C1, C2 = 26634, 239708                       # (0.01 * 255)^2 * 4096 and (0.03 * 255)^2 * 4096, rounded
DEFAULTS = dict(flags=SSIM | PROFILE, ring_width=16)
assert (C1, C2) == (round((0.01 * 255) ** 2 * 4096), round((0.03 * 255) ** 2 * 4096))


def as_int32(v):
    """(int64)(int32) of a gaze coordinate held as a uint32."""
    return ((int(v) & 0xffffffff) ^ 0x80000000) - 0x80000000


def classes_of_fill(fill, uniform):
    """The class of every pixel from the fill of its last writer (0: none) and the frame's FOV_OFF flag."""
    fill = np.asarray(fill)
    k = np.where(fill == 4, PERIPHERY, np.where(fill == 2, MIDDLE, FOVEA))
    if uniform:
        k = np.full(fill.shape, UNIFORM)
    return np.where(fill == 0, UNWRITTEN, k).astype(np.uint8)


def classes_of_frame(w, h, gaze, r_inner, r_outer, uniform):
    """The classes of a frame fovpt_render rendered with that gaze (uint32 values) and those radii."""
    import reconstruct_ref as rr
    return classes_of_fill(rr.writers(w, h, gaze, r_inner, r_outer, uniform)[0], uniform)


def channels(img):
    """(H, W) uint32 -> (H, W, 3) int64: R, G, B, the low three bytes; alpha is ignored."""
    img = np.asarray(img, np.uint32)
    return np.stack([(img >> (8 * c)) & 255 for c in range(3)], axis=-1).astype(np.int64)


def luma(img):
    c = channels(img)
    return (54 * c[..., 0] + 183 * c[..., 1] + 19 * c[..., 2] + 128) >> 8


def isqrt(d):
    """The floor square root of an int64 array of values below 2^53: the binary64 root corrected in integers."""
    d = np.asarray(d, np.int64)
    assert (d >= 0).all() and (d < (1 << 53)).all()
    r = np.floor(np.sqrt(d.astype(np.float64))).astype(np.int64)
    r -= (r * r > d)
    r += ((r + 1) * (r + 1) <= d)
    assert ((r * r <= d) & ((r + 1) * (r + 1) > d)).all()
    return r


def ring_map(w, h, gaze, ring_width):
    """min(63, isqrt(dx^2 + dy^2) / ring_width) per pixel, dx = x - (int64)(int32)gaze x.  |dx| or |dy| >= 2^22 is ring 63 whatever
    the other is (isqrt(d2) >= 2^22 > 63 * MAX_RING_WIDTH), which keeps d2 inside 64 bits for every gaze; ring_of() is the same
    statement in Python integers without that shortcut."""
    dx = np.abs(np.arange(w, dtype=np.int64) - as_int32(gaze[0]))[None, :]
    dy = np.abs(np.arange(h, dtype=np.int64) - as_int32(gaze[1]))[:, None]
    far = (dx >= (1 << 22)) | (dy >= (1 << 22))
    dx, dy = np.minimum(dx, 1 << 22), np.minimum(dy, 1 << 22)
    return np.where(far, RINGS - 1, np.minimum(RINGS - 1, isqrt(dx * dx + dy * dy) // int(ring_width)))


def ring_of(x, y, gaze, ring_width):
    """One pixel's ring in Python integers (math.isqrt): what ring_map states for a whole frame."""
    dx, dy = x - as_int32(gaze[0]), y - as_int32(gaze[1])
    return min(RINGS - 1, math.isqrt(dx * dx + dy * dy) // int(ring_width))


def window_q(T, F):
    """The windows of two luma images: (origins y, origins x, q) with q the (nj, ni) int64 array of the windows' scaled SSIM."""
    h, w = T.shape
    if w < 8 or h < 8:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 0), np.int64)
    from numpy.lib.stride_tricks import sliding_window_view
    ys, xs = np.arange(0, h - 7, 4), np.arange(0, w - 7, 4)
    a = sliding_window_view(T, (8, 8))[::4, ::4].astype(np.int64)
    b = sliding_window_view(F, (8, 8))[::4, ::4].astype(np.int64)
    sx, sy = a.sum(axis=(2, 3)), b.sum(axis=(2, 3))
    sxx, syy, sxy = (a * a).sum(axis=(2, 3)), (b * b).sum(axis=(2, 3)), (a * b).sum(axis=(2, 3))
    A = 2 * sx * sy + C1
    B = 2 * (64 * sxy - sx * sy) + C2
    C = sx * sx + sy * sy + C1
    D = (64 * sxx - sx * sx) + (64 * syy - sy * sy) + C2
    N, M = A * B, C * D
    assert (np.abs(N) < (1 << 57)).all() and (M > 0).all() and (M < (1 << 57)).all()
    q = np.rint((N.astype(np.float64) / M.astype(np.float64)) * 1048576.0).astype(np.int64)
    return ys, xs, q


def quality(test, ref, classes, gaze, cfg=None):
    """test, ref: (H, W) uint32 rgba8 images; classes: (H, W) class per pixel; gaze: (x, y), uint32 or signed values; cfg: flags and
    ring_width (DEFAULTS).  -> the fields of a fovpt_quality_sums as Python integers and lists (abi.QualitySums.as_dict())."""
    cfg = dict(DEFAULTS, **(cfg or {}))
    flags, rw = int(cfg["flags"]), int(cfg["ring_width"])
    assert flags & ~(SSIM | PROFILE) == 0 and 1 <= rw <= MAX_RING_WIDTH
    test, ref, classes = np.asarray(test, np.uint32), np.asarray(ref, np.uint32), np.asarray(classes)
    h, w = test.shape
    assert ref.shape == (h, w) and classes.shape == (h, w) and classes.max() < CLASSES
    d = channels(test) - channels(ref)
    sq, amax = d * d, np.abs(d).max(axis=-1)
    out = dict(pixels=[], differing=[], sq_err=[], max_err=[], _pad=0, windows=[0] * CLASSES, ssim_q20=[0] * CLASSES,
               ring_pixels=[0] * RINGS, ring_sq_err=[0] * RINGS, width=w, height=h, ring_width=rw, flags=flags)
    for k in range(CLASSES):
        m = classes == k
        out["pixels"].append(int(m.sum()))
        out["differing"].append(int((amax[m] != 0).sum()))
        out["sq_err"].append([int(sq[..., c][m].sum()) for c in range(3)])
        out["max_err"].append(int(amax[m].max()) if m.any() else 0)
    if flags & PROFILE:
        ring = ring_map(w, h, gaze, rw)
        tot = sq.sum(axis=-1)
        for r in range(RINGS):
            m = ring == r
            out["ring_pixels"][r] = int(m.sum())
            out["ring_sq_err"][r] = int(tot[m].sum())
    if flags & SSIM:
        ys, xs, q = window_q(luma(test), luma(ref))
        if q.size:
            kc = classes[np.ix_(ys + 4, xs + 4)]                 # the class of a window: that of pixel (x0 + 4, y0 + 4)
            for k in range(CLASSES):
                m = kc == k
                out["windows"][k] = int(m.sum())
                out["ssim_q20"][k] = int(q[m].sum())
    return out


# ---- the derived scores (fovpt_quality_mse / _psnr / _ssim / _score), binary64 -----------------------------------------------------
def _range(cls):
    return range(UNWRITTEN) if cls == -1 else range(cls, cls + 1)


def mse(s, cls=-1):
    sq = sum(sum(s["sq_err"][k]) for k in _range(cls))
    n = sum(s["pixels"][k] for k in _range(cls))
    return float(sq) / (3.0 * float(n)) if n else float("nan")


def psnr(s, cls=-1):
    m = mse(s, cls)
    if m != m:
        return m
    return float("inf") if m == 0.0 else 10.0 * math.log10(65025.0 / m)


def ssim(s, cls=-1):
    q = sum(s["ssim_q20"][k] for k in _range(cls))
    n = sum(s["windows"][k] for k in _range(cls))
    return float(q) / (1048576.0 * float(n)) if n else float("nan")


def score(s, weights):
    num = den = 0.0
    for k in range(CLASSES):
        num += float(weights[k]) * float(sum(s["sq_err"][k]))
        den += float(weights[k]) * float(s["pixels"][k])
    return num / (3.0 * den) if den > 0.0 else float("nan")
