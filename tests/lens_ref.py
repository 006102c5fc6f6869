"""fovpt_lens restated in numpy: the definition in include/fovpt.h, operation by operation.

float32 arrays throughout, every sum, difference, product and quotient one rounding, one operation per line; H in Python floats
(binary64) by the stated formula, each entry rounded to float32; the oracle's make_color (with and without the resolve's tone map)
for the rgba8.  w, h: the frame size; (x, y) a destination pixel.

    1  nx = (float)(2x + 1) / (float)w - 1, ny likewise with h
    2  px = (nx - center.x) * scale.x, py likewise; r2 = px * px + py * py
    3  !(r2 <= clip_r2): outside the lens, out_color = border (all four components)
    4  f = k0 + r2 * (k1 + r2 * (k2 + r2 * k3)); per channel c: fc = f * chroma[c], sx = (px * fc) * src_scale.x + src_center.x
    5  with `to`: a_k = (H[k][0] * sx + H[k][1] * sy) + H[k][2]; valid iff a.z > 0; sx = a.x / a.z, sy = a.y / a.z
    6  fx = ((sx + 1) * 0.5) * w - 0.5, fy likewise with h
    7  invalid (step 5, or !(fx >= -2 && fx <= w + 1), or the same in y): border[c], no tap is read
    8  NEAREST / BILINEAR / BICUBIC over taps that read border[c] outside the frame; a window with no tap inside it: border[c]
    9  out_color = (v_r, v_g, v_b, 1); out_rgba by `encode`"""
import ctypes as C

import numpy as np

import temporal_ref as tr

f32 = np.float32
NEAREST, BILINEAR, BICUBIC = 0, 1, 2
ENCODE_DISPLAY, ENCODE_RESOLVE = 0, 1
DEFAULTS = dict(filter=BILINEAR, encode=ENCODE_DISPLAY, center=(0.0, 0.0), scale=(1.0, 1.0), k=(1.0, 0.22, 0.24, 0.0),
                chroma=(0.996, 1.0, 1.014), clip_r2=float("inf"), src_center=(0.0, 0.0), src_scale=(1.0, 1.0), border=(0.0, 0.0, 0.0, 1.0))
TAPS = {NEAREST: 1, BILINEAR: 2, BICUBIC: 4}


def config(**replace):
    d = dict(DEFAULTS)
    d.update(replace)
    return d


def same_bits(values):
    b = np.asarray(values, np.float32).view(np.uint32)
    return bool((b == b[0]).all())


def poly(k, r2):
    """Step 4's f in float32."""
    k = [f32(v) for v in k]
    r2 = np.asarray(r2, np.float32)
    with np.errstate(all="ignore"):
        t = r2 * k[3]
        t = k[2] + t
        t = r2 * t
        t = k[1] + t
        t = r2 * t
        return (k[0] + t).astype(np.float32)


def homography(cam, to):
    """H = M [U_to V_to W_to] -> (3, 3) float32, or None for a singular rendered camera.  M: the float32 rows of inverse(U V W) of
    the rendered camera (temporal_ref.camera_inverse); each entry (m0 * b0 + m1 * b1) + m2 * b2 in binary64, then rounded."""
    M = tr.camera_inverse(cam["U"], cam["V"], cam["W"])
    if M is None:
        return None
    cols = [[float(f32(v)) for v in to[n]] for n in ("U", "V", "W")]
    H = np.zeros((3, 3), np.float32)
    for k in range(3):
        m = [float(M[k, i]) for i in range(3)]
        for j in range(3):
            b = cols[j]
            H[k, j] = f32((m[0] * b[0] + m[1] * b[1]) + m[2] * b[2])
    return H


def cubic_weights(t):
    t = np.asarray(t, np.float32)
    w0 = f32(-0.5) * t
    w0 = w0 + f32(1.0)
    w0 = w0 * t
    w0 = w0 - f32(0.5)
    w0 = w0 * t
    w1 = f32(1.5) * t
    w1 = w1 - f32(2.5)
    w1 = w1 * t
    w1 = w1 * t
    w1 = w1 + f32(1.0)
    w2 = f32(-1.5) * t
    w2 = w2 + f32(2.0)
    w2 = w2 * t
    w2 = w2 + f32(0.5)
    w2 = w2 * t
    w3 = f32(0.5) * t
    w3 = w3 - f32(0.5)
    w3 = w3 * t
    w3 = w3 * t
    return [np.asarray(x, np.float32) for x in (w0, w1, w2, w3)]


def _position(d, H, w, h, px, py, f, chroma):
    """Steps 4 to 7 for one chroma factor -> (valid, fx, fy, front: step 5's a.z > 0, all True without a re-aim)."""
    fw, fh = f32(w), f32(h)
    with np.errstate(all="ignore"):
        fc = f * f32(chroma)
        sx = px * fc
        sx = sx * f32(d["src_scale"][0])
        sx = sx + f32(d["src_center"][0])
        sy = py * fc
        sy = sy * f32(d["src_scale"][1])
        sy = sy + f32(d["src_center"][1])
        front = np.ones(px.shape, bool)
        if H is not None:
            a = []
            for k in range(3):
                t0 = H[k, 0] * sx
                t1 = H[k, 1] * sy
                t = t0 + t1
                a.append(t + H[k, 2])
            front = a[2] > 0
            sx = a[0] / a[2]
            sy = a[1] / a[2]
        fx = sx + f32(1.0)
        fx = fx * f32(0.5)
        fx = fx * fw
        fx = fx - f32(0.5)
        fy = sy + f32(1.0)
        fy = fy * f32(0.5)
        fy = fy * fh
        fy = fy - f32(0.5)
        hi_x = fw + f32(1.0)
        hi_y = fh + f32(1.0)
        valid = front & (fx >= f32(-2.0)) & (fx <= hi_x) & (fy >= f32(-2.0)) & (fy <= hi_y)
    assert fx.dtype == np.float32 and fy.dtype == np.float32
    return valid, fx, fy, front


def _filter(d, color, c, valid, fx, fy):
    """Step 8 for channel c -> (v float32, x0, y0 int64: the window's first tap, border_taps int64)."""
    h, w = color.shape[:2]
    flt = d["filter"]
    n = TAPS[flt]
    b = f32(d["border"][c])
    fx = np.where(valid, fx, f32(0.0)).astype(np.float32)                  # (an invalid channel reads no tap: any position will do)
    fy = np.where(valid, fy, f32(0.0)).astype(np.float32)
    if flt == NEAREST:
        flx, fly = np.floor(fx + f32(0.5)), np.floor(fy + f32(0.5))
    else:
        flx, fly = np.floor(fx), np.floor(fy)
    tx, ty = fx - flx, fy - fly
    x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
    if flt == BICUBIC:
        x0, y0 = x0 - 1, y0 - 1
    taps = [[None] * n for _ in range(n)]
    border_taps = np.zeros(fx.shape, np.int64)
    for j in range(n):
        for i in range(n):
            qx, qy = x0 + i, y0 + j
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            border_taps += ~inside
            taps[j][i] = np.where(inside, color[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1), c], b).astype(np.float32)
    with np.errstate(all="ignore"):
        if flt == NEAREST:
            v = taps[0][0]
        elif flt == BILINEAR:
            ux = f32(1.0) - tx
            uy = f32(1.0) - ty
            top = ux * taps[0][0] + tx * taps[0][1]
            bottom = ux * taps[1][0] + tx * taps[1][1]
            v = uy * top + ty * bottom
        else:
            wx, wy = cubic_weights(tx), cubic_weights(ty)
            rows = []
            for j in range(4):
                r = wx[0] * taps[j][0] + wx[1] * taps[j][1]
                r = r + wx[2] * taps[j][2]
                r = r + wx[3] * taps[j][3]
                rows.append(r)
            v = wy[0] * rows[0] + wy[1] * rows[1]
            v = v + wy[2] * rows[2]
            v = v + wy[3] * rows[3]
            v = np.where(v < f32(0.0), f32(0.0), v)
    v = np.where(border_taps < n * n, v, b)                                # a window with no tap inside the frame: the border, exactly
    v = np.where(valid, v, b).astype(np.float32)
    border_taps = np.where(valid, border_taps, 0)
    return v, x0, y0, border_taps


def make_color_raw(oracle, rgb):
    rgb = np.ascontiguousarray(rgb, np.float32)
    out = np.empty(rgb.shape[0], np.uint32)
    oracle.lib().orc_make_color_raw(C.c_int(rgb.shape[0]), rgb.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


def lens(oracle, color, d, cam=None, to=None, share=True):
    """One fovpt_lens call on the (h, w, 4) float32 frame `color` -> dict(color (h, w, 4), rgba (h, w) uint32 (None without an
    oracle), inside (h, w) bool: inside the lens, valid (h, w, 3) bool, front (h, w, 3) bool: step 5's a.z > 0, fx, fy (h, w, 3) float32, x0, y0 (h, w, 3) int64: the first
    tap of each channel's window (meaningful where valid), border_taps (h, w, 3): taps of a valid channel's window outside the
    frame, H).  d: a full config dict; cam / to: dicts of U / V / W of the rendered and of the late camera (to None: no re-aim).
    share: where the three chroma factors have equal bits, evaluate one position and use it for the three channels, as the kernel
    does; False evaluates every channel on its own."""
    color = np.ascontiguousarray(color, np.float32)
    h, w = color.shape[:2]
    H = homography(cam, to) if to is not None else None
    assert to is None or H is not None, "a singular rendered camera is refused by the library"
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        nx = (2 * xs + 1).astype(np.float32) / f32(w)
        nx = nx - f32(1.0)
        ny = (2 * ys + 1).astype(np.float32) / f32(h)
        ny = ny - f32(1.0)
        px = nx - f32(d["center"][0])
        px = px * f32(d["scale"][0])
        py = ny - f32(d["center"][1])
        py = py * f32(d["scale"][1])
        r2 = px * px + py * py
        inside = r2 <= f32(d["clip_r2"])
    f = poly(d["k"], r2)
    out = np.empty((h, w, 4), np.float32)
    valid = np.zeros((h, w, 3), bool)
    fxs, fys = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32)
    x0s, y0s = np.zeros((h, w, 3), np.int64), np.zeros((h, w, 3), np.int64)
    bts = np.zeros((h, w, 3), np.int64)
    fronts = np.zeros((h, w, 3), bool)
    mono = share and same_bits(d["chroma"])
    pos = None
    for c in range(3):
        if pos is None or not mono:
            pos = _position(d, H, w, h, px, py, f, d["chroma"][c])
        ok, fx, fy, front = pos
        ok = ok & inside
        fronts[..., c] = front
        v, x0, y0, bt = _filter(d, color, c, ok, fx, fy)
        out[..., c] = v
        valid[..., c], fxs[..., c], fys[..., c], x0s[..., c], y0s[..., c], bts[..., c] = ok, fx, fy, x0, y0, bt
    out[..., 3] = 1.0
    out[~inside] = np.asarray(d["border"], np.float32)
    rgba = None
    if oracle is not None:
        rgb = np.ascontiguousarray(out[..., :3].reshape(-1, 3))
        rgba = (oracle.make_color(rgb) if d["encode"] == ENCODE_RESOLVE else make_color_raw(oracle, rgb)).reshape(h, w)
    return dict(color=out, rgba=rgba, inside=inside, valid=valid, fx=fxs, fy=fys, x0=x0s, y0=y0s, border_taps=bts, front=fronts, H=H)
