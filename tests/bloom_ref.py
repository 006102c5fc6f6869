"""fovpt_bloom restated in numpy: the definition in include/fovpt.h, operation by operation.

numpy float32 throughout, every product, sum, difference and quotient one rounding; min(a, b) = a < b ? a : b and max likewise
(np.where on the comparison); the oracle's make_color for the rgba8.  The level sizes and the packed layout of the pyramid are
here too (level_sizes, level_offsets, pack)."""
import numpy as np

f32 = np.float32
MAX_LEVELS = 8
KARIS, GAINS, EXPOSURE_STATE = 1, 2, 4
DEFAULTS = dict(flags=KARIS, levels=6, threshold=1.0, knee=0.5, exposure=16.0, intensity=0.05, spread=0.7,
                gain_fovea=1.0, gain_middle=1.0, gain_periphery=1.0, gain_uniform=1.0)


def level_sizes(w, h, n):
    """[(W_k, H_k)] for k = 0 .. n - 1: W_k = ceil(W_{k-1} / 2) from W_{-1} = w (a 1-wide level stays 1 wide)."""
    out = []
    for _ in range(n):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out


def level_offsets(w, h, n):
    """The first texel of each level in the packed pyramid, and behind them the total: n + 1 entries."""
    off = [0]
    for W, H in level_sizes(w, h, n):
        off.append(off[-1] + W * H)
    return off


def pack(levels):
    """The levels ((H_k, W_k, 4) each) as the pyramid holds them: (texels, 4), one level after the other, rows first."""
    return np.concatenate([np.asarray(l, np.float32).reshape(-1, 4) for l in levels], axis=0)


def fmin(a, b):
    return np.where(a < b, a, b)


def fmax(a, b):
    return np.where(a > b, a, b)


def luminance(c):
    return (f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]


def constants(d, E):
    """Step 0 -> (T, K, K2, K4) as float32."""
    E = f32(E)
    T, K = f32(d["threshold"]) / E, f32(d["knee"]) / E
    return T, K, f32(2.0) * K, f32(4.0) * K


def gains(fill, d, uniform):
    """GAINS: the gain of each pixel from the fill of its last writer (0: no writer; reconstruct_ref.writers)."""
    fill = np.asarray(fill)
    if uniform:
        g = np.where(fill > 0, f32(d["gain_uniform"]), f32(0))
    else:
        g = np.select([fill == 0, fill == 4, fill == 2], [f32(0), f32(d["gain_periphery"]), f32(d["gain_middle"])], f32(d["gain_fovea"]))
    return g.astype(np.float32)


def bright(c, T, K, K2, K4):
    """Step 1's L and m of pixels (..., >= 3)."""
    zero = f32(0)
    L = luminance(c)
    s = fmax(zero, fmin(L - (T - K), K2))
    q = (s * s) / K4 if K > 0 else np.zeros_like(L)
    m = fmax(fmax(q, L - T), zero) / fmax(L, f32(1e-6))
    return L, m.astype(np.float32)


def prefilter(color, d, E, fill=None, uniform=0):
    """Step 1 -> d_0 (H_0, W_0, 4), the fourth channel 0.  fill: the frame's last-writer fills (GAINS only)."""
    color = np.asarray(color, np.float32)
    h, w = color.shape[:2]
    (W0, H0), = level_sizes(w, h, 1)
    T, K, K2, K4 = constants(d, E)
    g_px = gains(fill, d, uniform) if d["flags"] & GAINS else np.ones((h, w), np.float32)
    num = np.zeros((H0, W0, 3), np.float32)
    den = np.zeros((H0, W0), np.float32)
    X, Y = np.arange(W0), np.arange(H0)
    with np.errstate(all="ignore"):
        for j in (0, 1):
            py = np.minimum(2 * Y + j, h - 1)
            for i in (0, 1):
                px = np.minimum(2 * X + i, w - 1)
                c = color[py][:, px, :3]
                L, m = bright(c, T, K, K2, K4)
                kw = f32(1.0) / (f32(1.0) + L) if d["flags"] & KARIS else np.ones_like(L)
                wt = g_px[py][:, px] * kw
                num = num + wt[..., None] * (c * m[..., None])
                den = den + kw
        out = np.zeros((H0, W0, 4), np.float32)
        out[..., :3] = num / den[..., None]
    return out


def downsample(S):
    """Step 2: the level below S ((Hs, Ws, 4))."""
    S = np.asarray(S, np.float32)
    Hs, Ws = S.shape[:2]
    (W, H), = level_sizes(Ws, Hs, 1)
    X, Y = np.arange(W), np.arange(H)
    b = (1, 3, 3, 1)
    acc = np.zeros((H, W, 3), np.float32)
    for j in range(4):
        sy = np.clip(2 * Y - 1 + j, 0, Hs - 1)
        for i in range(4):
            sx = np.clip(2 * X - 1 + i, 0, Ws - 1)
            wgt = f32(b[j] * b[i]) * f32(0.015625)
            acc = acc + wgt * S[sy][:, sx, :3]
    out = np.zeros((H, W, 4), np.float32)
    out[..., :3] = acc
    return out


def upsample(S, W, H):
    """Step 3: up(S)(x, y) for x < W, y < H -> (H, W, 3)."""
    S = np.asarray(S, np.float32)[..., :3]
    Hs, Ws = S.shape[:2]
    x, y = np.arange(W), np.arange(H)
    ax, ay = x >> 1, y >> 1
    bx = np.clip(np.where(x & 1, ax + 1, ax - 1), 0, Ws - 1)
    by = np.clip(np.where(y & 1, ay + 1, ay - 1), 0, Hs - 1)
    a, q = f32(0.75), f32(0.25)
    r0 = a * S[ay][:, ax] + q * S[ay][:, bx]
    r1 = a * S[by][:, ax] + q * S[by][:, bx]
    return a * r0 + q * r1


def pyramid(d0, n, spread):
    """Steps 2 and 4 from d_0 -> (the d_k, the u_k), n levels each."""
    ds = [np.asarray(d0, np.float32)]
    for _ in range(1, n):
        ds.append(downsample(ds[-1]))
    us = [None] * n
    us[n - 1] = ds[n - 1]
    for k in range(n - 2, -1, -1):
        H, W = ds[k].shape[:2]
        u = np.zeros_like(ds[k])
        u[..., :3] = ds[k][..., :3] + f32(spread) * upsample(us[k + 1], W, H)
        us[k] = u
    return ds, us


def composite(color, u0, intensity):
    """Step 5's float colour."""
    color = np.asarray(color, np.float32)
    h, w = color.shape[:2]
    out = color.copy()
    with np.errstate(all="ignore"):
        out[..., :3] = color[..., :3] + f32(intensity) * upsample(u0, w, h)
    return out


def bloom(oracle, color, d, E=None, fill=None, uniform=0):
    """One fovpt_bloom call -> dict(color (h, w, 4), rgba (h, w) or None without an oracle, d: the d_k, u: the u_k, pyramid: what
    the call leaves in memory).  d: a full config dict (DEFAULTS with replacements); E: the exposure of step 0 (None:
    d["exposure"]; the caller resolves EXPOSURE_STATE)."""
    color = np.asarray(color, np.float32)
    E = f32(d["exposure"]) if E is None else f32(E)
    d0 = prefilter(color, d, E, fill, uniform)
    ds, us = pyramid(d0, d["levels"], d["spread"])
    out = composite(color, us[0], d["intensity"])
    rgba = None
    if oracle is not None:
        rgba = oracle.make_color(np.ascontiguousarray(out[..., :3].reshape(-1, 3))).reshape(color.shape[:2])
    return dict(color=out, rgba=rgba, d=ds, u=us, pyramid=pack(us))
