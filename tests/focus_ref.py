"""fovpt_focus restated in numpy: the definition in include/fovpt.h, operation by operation.

numpy / Python integers for the disc, the bins, the histogram and the rank (step 1), numpy float32 for the adapt step, the radii and
the gather (steps 2 to 4: every sum, difference, product and quotient one rounding), and the oracle's make_color for the rgba8.
The gather vectorises over pixels and loops over the (2 max_radius + 1)^2 taps in the definition's order, so every pixel's running
sums are added in visiting order."""
import numpy as np

f32 = np.float32
FIXED, AUTO = 0, 1
MAX_RADIUS, MAX_METER_RADIUS, BINS = 8, 64, 256
MISS = 0xffffffff
TILE = (32, 16)                 # outputs of a block of k_focus_gather (w, h): the kernel's shortcuts are per tile
DEFAULTS = dict(mode=AUTO, meter_radius=12, rank_permille=250, max_radius=6, strength=8.0, focus_distance=1.0, focus_default=1.0,
                adapt_nearer=1.0, adapt_farther=1.0)


def config(**replace):
    d = dict(DEFAULTS)
    d.update(replace)
    return d


def new_state():
    return dict(focus_metered=f32(0), inv_focus=f32(0), focus=f32(0), count=0, steps=0)


def bin_centre(b):
    """The float whose bits are ((b + 888) << 20) | 0x80000."""
    return np.array([((int(b) + 888) << 20) | 0x80000], np.uint32).view(np.float32)[0]


def histogram(prim, t, gaze, meter_radius):
    """Step 1's histogram -> (256,) int64.  prim (h, w) uint32, t (h, w) float32, gaze (cx, cy) as Python integers."""
    prim, t = np.asarray(prim), np.ascontiguousarray(t, np.float32)
    h, w = prim.shape
    cx, cy = int(gaze[0]), int(gaze[1])
    hist = np.zeros(BINS, np.int64)
    R = int(meter_radius)
    x0, x1, y0, y1 = max(cx - R, 0), min(cx + R, w - 1), max(cy - R, 0), min(cy + R, h - 1)
    if x0 > x1 or y0 > y1:
        return hist
    ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
    inside = (xs - cx) ** 2 + (ys - cy) ** 2 <= R * R
    tt = t[y0:y1 + 1, x0:x1 + 1]
    with np.errstate(invalid="ignore"):
        counts = inside & (prim[y0:y1 + 1, x0:x1 + 1] != MISS) & (tt > 0)
    u = np.ascontiguousarray(tt).view(np.uint32).astype(np.int64)
    b = np.clip((u >> 20) - 888, 0, BINS - 1)
    np.add.at(hist, b[counts], 1)
    return hist


def rank_bin(hist, rank_permille):
    """-> (b or None when T == 0, T).  Python integers."""
    hist = [int(x) for x in hist]
    T = sum(hist)
    if T == 0:
        return None, 0
    k = min(T * int(rank_permille) // 1000, T - 1)
    run = 0
    for b, n in enumerate(hist):
        run += n
        if run > k:
            return b, T
    raise AssertionError("unreachable")


def adapt(state, hist, d):
    """Steps 1 (rank) and 2 -> the new state."""
    b, T = rank_bin(hist, d["rank_permille"])
    first = state["steps"] == 0
    D = f32(state["inv_focus"])
    with np.errstate(all="ignore"):
        if b is not None:
            metered = bin_centre(b)
            Dm = f32(1.0) / metered
        elif first:
            metered = f32(d["focus_default"])
            Dm = f32(1.0) / metered
        else:
            metered, Dm = f32(state["focus"]), D                 # nothing to meter: the present focus, D stays
        if first:
            D = Dm
        else:
            rate = f32(d["adapt_nearer"]) if Dm > D else f32(d["adapt_farther"])
            D = f32(D + f32(rate * f32(Dm - D)))
        focus = f32(1.0) / D
    return dict(focus_metered=f32(metered), inv_focus=f32(D), focus=f32(focus), count=T, steps=state["steps"] + 1)


def radius(prim, t, D, d):
    """Step 3 -> (r, tp), (h, w) float32 each."""
    t = np.asarray(t, np.float32)
    hit = np.asarray(prim) != MISS
    with np.errstate(all="ignore"):
        i = np.where(hit, f32(1.0) / t, f32(0.0)).astype(np.float32)
        s = f32(d["strength"]) * np.abs(i - f32(D))
        cap = f32(d["max_radius"])
        r = np.where(s < cap, s, cap).astype(np.float32)
    tp = np.where(hit, t, f32(np.inf)).astype(np.float32)
    return r, tp


def _shifted(a, dx, dy, fill):
    """a[y + dy, x + dx] where that is inside the frame, `fill` elsewhere."""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    ys0, ys1 = max(0, -dy), min(h, h - dy)
    xs0, xs1 = max(0, -dx), min(w, w - dx)
    if ys0 < ys1 and xs0 < xs1:
        out[ys0:ys1, xs0:xs1] = a[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]
    return out


def gather(color, r, tp, max_radius, bound=None):
    """Step 4 -> (out_color (h, w, 4), covering (h, w) int, acted (h, w) bool: some tap inside the frame had re < rq -- the
    background rule acted --, cut (h, w) bool: some tap of the window was outside the frame).  bound: None, or an (h, w) int array
    that restricts a pixel's taps to |dx|, |dy| <= bound (the kernel's tile-wise loop bound, for the check that it changes nothing)."""
    color = np.asarray(color, np.float32)
    h, w = r.shape
    R = int(max_radius)
    den = np.zeros((h, w), np.float32)
    num = np.zeros((h, w, 3), np.float32)
    covering = np.zeros((h, w), np.int64)
    acted = np.zeros((h, w), bool)
    cut = np.zeros((h, w), bool)
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                inside = (xs + dx >= 0) & (xs + dx < w) & (ys + dy >= 0) & (ys + dy < h)
                cut |= ~inside
                if bound is not None:
                    inside = inside & (bound >= max(abs(dx), abs(dy)))
                rq, tq = _shifted(r, dx, dy, f32(0)), _shifted(tp, dx, dy, f32(0))
                cq = _shifted(color[..., :3], dx, dy, f32(0))
                behind = tq > tp
                re = np.where(behind, np.where(rq < r, rq, r), rq).astype(np.float32)
                e = re + f32(0.5)
                e2 = e * e
                covers = inside & (f32(dx * dx + dy * dy) <= e2)
                acted |= inside & (re < rq)
                g = f32(1.0) / e2
                den = np.where(covers, den + g, den).astype(np.float32)
                num = np.where(covers[..., None], num + g[..., None] * cq, num).astype(np.float32)
                covering += covers
        out = color.copy()
        blur = covering > 1
        out[..., :3] = np.where(blur[..., None], num / den[..., None], color[..., :3])
    return out, covering, acted, cut


def tile_bounds(r, max_radius, tile=TILE):
    """k_focus_gather's loop bound per pixel: min(max_radius, floor(m + 0.5f)), m the largest r of the pixel's tile and its apron
    of max_radius pixels inside the frame, the sum in float32.  0: the tile is a copy."""
    h, w = r.shape
    R = int(max_radius)
    out = np.zeros((h, w), np.int64)
    for ty in range(0, h, tile[1]):
        for tx in range(0, w, tile[0]):
            m = r[max(ty - R, 0):min(ty + tile[1] + R, h), max(tx - R, 0):min(tx + tile[0] + R, w)].max()
            out[ty:ty + tile[1], tx:tx + tile[0]] = min(R, int(np.floor(f32(f32(m) + f32(0.5)))))
    return out


def focus(oracle, gb, gaze, color, d, state):
    """One fovpt_focus call -> dict(color, rgba (None without an oracle), coc, state, covering, acted, cut, tp).  gb: dict(prim (h, w)
    uint32, position (h, w, 4) float32); gaze: (cx, cy) unsigned as rendered; d: a full config dict; state: new_state() or what
    the previous call returned (FIXED returns it unchanged)."""
    prim = np.asarray(gb["prim"])
    t = np.ascontiguousarray(np.asarray(gb["position"], np.float32)[..., 3])
    if d["mode"] == AUTO:
        state = adapt(state, histogram(prim, t, gaze, d["meter_radius"]), d)
        D = state["inv_focus"]
    else:
        with np.errstate(all="ignore"):
            D = f32(1.0) / f32(d["focus_distance"])
    r, tp = radius(prim, t, D, d)
    out, covering, acted, cut = gather(color, r, tp, d["max_radius"])
    rgba = None
    if oracle is not None:
        rgba = oracle.make_color(np.ascontiguousarray(out[..., :3].reshape(-1, 3))).reshape(prim.shape)
    return dict(color=out, rgba=rgba, coc=r, state=state, covering=covering, acted=acted, cut=cut, tp=tp)
