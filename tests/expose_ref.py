"""fovpt_expose restated in numpy: the definition in include/fovpt.h, operation by operation.

numpy integers for the bins, the histogram and the trimmed mean (steps 2 to 4), numpy float32 for the luminance, the adaptation
and the tone map (steps 1, 5 and 7, every product, sum and quotient one rounding), binary64 for the mean of step 4, and the
oracle's deterministic powf and make_color for the exposure and the rgba8."""
import ctypes as C

import numpy as np

f32 = np.float32
FIXED, AUTO = 0, 1
FRAME, GAZE = 0, 1
REINHARD, ACES = 0, 1
BINS = 256
OP_POW = 6                      # FOVPT_OP_POW
DEFAULTS = dict(mode=AUTO, metering=GAZE, tone=REINHARD, weight_fovea=64, weight_middle=8, weight_periphery=1, weight_uniform=1,
                low_permille=100, high_permille=950, ev_min=-12.0, ev_max=12.0, key=0.18, exposure=16.0, white=1e6,
                adapt_brighter=1.0, adapt_darker=1.0)


def luminance(c):
    """Step 1, on (..., >= 3) float32."""
    c = np.asarray(c, np.float32)
    with np.errstate(all="ignore"):
        return (f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]


def bins(L):
    """Step 2 -> (counts: bool, bin: int64) per element."""
    L = np.ascontiguousarray(L, np.float32)
    with np.errstate(invalid="ignore"):
        counts = L > 0
    u = L.view(np.uint32).astype(np.int64)
    return counts, np.clip((u >> 20) - 888, 0, BINS - 1)


def weights(fill, d, uniform):
    """Step 3's GAZE weights from the fill of each pixel's last writer (0: no writer; reconstruct_ref.writers)."""
    fill = np.asarray(fill)
    if uniform:
        w = np.where(fill > 0, d["weight_uniform"], 0)
    else:
        w = np.select([fill == 1, fill == 2, fill == 4], [d["weight_fovea"], d["weight_middle"], d["weight_periphery"]], 0)
    return w.astype(np.int64)


def histogram(color, d, fill=None, uniform=0):
    """Steps 1 to 3 -> (256,) uint64.  fill: the frame's last-writer fills (GAZE only)."""
    counts, b = bins(luminance(color).reshape(-1))
    w = weights(fill, d, uniform).reshape(-1) if d["metering"] == GAZE else np.ones(b.shape, np.int64)
    h = np.zeros(BINS, np.int64)
    np.add.at(h, b[counts], w[counts])
    return h.astype(np.uint64)


def trimmed_mean(h, d):
    """Step 4 -> (ev_metered as float32 or None when N == 0, T).  Python integers: no width to overflow."""
    h = [int(x) for x in h]
    T = sum(h)
    a, b = T * int(d["low_permille"]) // 1000, (T * int(d["high_permille"]) + 999) // 1000
    N = b - a
    if N == 0:
        return None, T
    S, cum = 0, 0
    for k in range(BINS):
        c = max(0, min(cum + h[k], b) - max(cum, a))
        S += c * (2 * k + 1)
        cum += h[k]
    assert S < 1 << 53 and N < 1 << 52                         # (the conversions to binary64 are exact)
    m = np.float64(-16.0) + (np.float64(S) / (np.float64(2.0) * np.float64(N))) / np.float64(8.0)
    m = max(np.float64(f32(d["ev_min"])), min(m, np.float64(f32(d["ev_max"]))))
    return f32(m), T


def new_state():
    return dict(ev_metered=f32(0), ev=f32(0), exposure=f32(0), weight_total=0, steps=0)


def adapt(oracle, state, h, d):
    """Steps 4 to 6 on the state of the previous step -> the new state."""
    target, T = trimmed_mean(h, d)
    first = state["steps"] == 0
    ev = f32(state["ev"])
    if target is None:
        target = max(f32(d["ev_min"]), min(f32(0.0), f32(d["ev_max"]))) if first else ev
    if first:
        ev = target
    else:
        rate = f32(d["adapt_brighter"]) if target > ev else f32(d["adapt_darker"])
        ev = f32(ev + f32(rate * f32(target - ev)))
    p = oracle.math_op(OP_POW, np.float32([2.0]), np.float32([ev]))[0]
    with np.errstate(all="ignore"):
        E = f32(d["key"]) / p
    return dict(ev_metered=f32(target), ev=f32(ev), exposure=f32(E), weight_total=T, steps=state["steps"] + 1)


def make_color_raw(oracle, rgb):
    """make_color alone (oracle: orc_make_color_raw) of (n, 3) float32 -> (n,) uint32."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    out = np.empty(rgb.shape[0], np.uint32)
    oracle.lib().orc_make_color_raw(C.c_int(rgb.shape[0]), rgb.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


def tone(color, E, d):
    """Step 7's float colour: (..., 4) float32 with alpha 1."""
    c = np.asarray(color, np.float32)[..., :3]
    E = f32(E)
    with np.errstate(all="ignore"):
        x = c * E
        if d["tone"] == ACES:
            o = (x * (f32(2.51) * x + f32(0.03))) / (x * (f32(2.43) * x + f32(0.59)) + f32(0.14))
        else:                                                    # reinhard(x, white) of fovpt_pixel.h, with its 1.0f / s multiply
            lum = (f32(0.2126) * x[..., 0] + f32(0.7152) * x[..., 1]) + f32(0.0722) * x[..., 2]
            inv = f32(1.0) / (f32(1.0) + lum / f32(d["white"]))
            o = (x * f32(1.0)) * inv[..., None]
    out = np.empty(c.shape[:-1] + (4,), np.float32)
    out[..., :3] = o
    out[..., 3] = 1.0
    return out


def expose(oracle, color, d, state, fill=None, uniform=0):
    """One fovpt_expose call -> (out_color (..., 4), out_rgba (...), histogram or None, the new state).  d: a full config dict
    (DEFAULTS with replacements); state: new_state() or what the previous call returned (FIXED returns it unchanged)."""
    color = np.asarray(color, np.float32)
    h = None
    if d["mode"] == AUTO:
        h = histogram(color, d, fill, uniform)
        state = adapt(oracle, state, h, d)
        E = state["exposure"]
    else:
        E = f32(d["exposure"])
    out = tone(color, E, d)
    rgba = make_color_raw(oracle, out[..., :3].reshape(-1, 3)).reshape(color.shape[:-1])
    return out, rgba, h, state
