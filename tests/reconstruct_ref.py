"""numpy float32 restatement of fovpt_gbuffer's rays and fovpt_reconstruct (csrc/reconstruct.hip): the definition the GPU
kernels match bit for bit.

Every operation below is one IEEE binary32 operation in the order the kernels perform it (the library is built with
-ffp-contract=off, so the device does not fuse any of them either).

    writer  each pixel's last writer among the frame's passes (P, M, F; within a pass the launch index that comes last,
            ascending y then x): its fill f (4, 2, 1) and its anchor a = (ix, iy), the launch's sample pixel
    level   f == 2: bit 0 of levels, f == 4: bit 1; no writer, f == 1 or the level off -> out = in, bit for bit
    taps    q = clamp(a + (i f, j f), 0, size - 1), j = -1..1 (outer), i = -1..1 (inner)
    h(d)    max(0, 1 - |d| * inv_s),  inv_s = 1 / (support * f)
    e(s)    max(0, 1 - s)^2
    w_n     e(|N_q - N_p|^2 * inv_n)
    w_z     e(((dot(N_p, X_q - X_p)^2) * inv_z) / t_p^2)           N, X, t: the G-buffer's normal, position, t
            (p and q both misses: w_n = w_z = 1; exactly one a miss: 0)
    w       ((h(px - qx) * h(py - qy)) * w_n) * w_z
    D(A)    (A.x + A.y + A.z > 0) ? max(A, 1/64) : 1               as the denoiser's
    I_q     in(q) / D(albedo guide(q))  (remodulate = 1),  in(q)  (0)
    out     (sum w I_q / sum w) * D(G-buffer albedo(p))  (remodulate = 1, else without the factor), alpha 1; sum w == 0: in(p)
    rgba8   make_color(reinhard(out * 16, 1)) for every pixel (the resolve's tone map)

inv_s, inv_n, inv_z are computed once in float32 (the library does the same on the host)."""
import numpy as np

f32 = np.float32
DEFAULTS = dict(support=2.0, normal_sigma=0.5, depth_sigma=0.05, levels=3, remodulate=1)
MISS = np.uint32(0xffffffff)


def inv_sq(sigma):
    s = f32(sigma)
    return f32(1.0) / (s * s)


def _e(d):
    t = np.maximum(f32(0.0), f32(1.0) - d)
    return t * t


def _sq(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def demod(a):
    a = a[..., :3]
    s = (a[..., 0] + a[..., 1]) + a[..., 2]
    return np.where((s > 0)[..., None], np.maximum(a, f32(1.0 / 64)), f32(1.0))


def frame_passes(w, h, gaze, r_inner, r_outer, uniform):
    """The passes fovpt_render runs (frame_passes in fovpt_api.hip): (grid w, grid h, factor, fill, offset x, offset y,
    ring r_inner, ring r_outer) in launch order; offsets wrap as uint32."""
    if uniform:
        return [(w, h, 1, 1, 0, 0, 0.0, 1e9)]
    cx, cy = gaze
    m, f = r_outer + 2, r_inner + 1
    u32 = lambda v: v & 0xffffffff
    return [(w // 4, h // 4, 4, 4, 0, 0, float(r_outer), 1e9),
            (m, m, 2, 2, u32(cx - m), u32(cy - m), float(r_inner), float(m)),
            (2 * f, 2 * f, 1, 1, u32(cx - f), u32(cy - f), 0.0, float(f))]


def writers(w, h, gaze, r_inner, r_outer, uniform):
    """(fill, pass, anchor x, anchor y) per pixel of its last writer: every launch index that passes the ring test (on its
    block's top-left pixel) writes its fill x fill block, clamped onto the frame's last row / column (pixel indices are uint32
    sums, so a block at a wrapped index 0xffffffff also covers pixel 0); the highest pass wins,
    within a pass the launch index that comes last.  fill 0 / pass -1: no writer.  Anchors are the uint32 values."""
    best = np.full((h, w), -1, np.int64)
    passes = frame_passes(w, h, gaze, r_inner, r_outer, uniform)
    cx, cy = gaze
    for p, (gw, gh, fac, fl, ox, oy, r_in, r_out) in enumerate(passes):
        ly, lx = np.mgrid[0:gh, 0:gw].astype(np.int64)
        ix = (lx * fac + ox) & 0xffffffff
        iy = (ly * fac + oy) & 0xffffffff
        dx = ix.astype(np.float32) - f32(cx)
        dy = iy.astype(np.float32) - f32(cy)
        rng = np.sqrt((dx * dx + dy * dy) + f32(0.0))
        alive = ~((rng < f32(r_in)) | (rng > f32(r_out)))
        key = (np.int64(p) << 40) | (ly * gw + lx)
        ix, iy, key = ix[alive], iy[alive], key[alive]
        for v in range(fl):
            for u in range(fl):
                np.maximum.at(best, (np.minimum((iy + v) & 0xffffffff, h - 1), np.minimum((ix + u) & 0xffffffff, w - 1)), key)
    fill = np.zeros((h, w), np.int64)
    pas = np.full((h, w), -1, np.int64)
    ax = np.zeros((h, w), np.int64)
    ay = np.zeros((h, w), np.int64)
    has = best >= 0
    for p, (gw, gh, fac, fl, ox, oy, _, _) in enumerate(passes):
        sel = has & ((best >> 40) == p)
        li = best[sel] & ((1 << 40) - 1)
        fill[sel] = fl
        pas[sel] = p
        ax[sel] = ((li % gw) * fac + ox) & 0xffffffff
        ay[sel] = ((li // gw) * fac + oy) & 0xffffffff
    return fill, pas, ax, ay


def primary_rays(w, h, eye, U, V, W):
    """fovpt_gbuffer's rays: generate_rays' expression with jitter 0.5 -> origins, directions (h * w, 3) float32."""
    y, x = np.mgrid[0:h, 0:w]
    dx = f32(2.0) * ((x.astype(np.float32) + f32(0.5)) / f32(w)) - f32(1.0)
    dy = f32(2.0) * ((y.astype(np.float32) + f32(0.5)) / f32(h)) - f32(1.0)
    U, V, W = (np.asarray(v, np.float32) for v in (U, V, W))
    d = (dx[..., None] * U + dy[..., None] * V) + W
    inv = f32(1.0) / np.sqrt(_dot(d, d))
    d = (d * inv[..., None]).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(eye, np.float32), d.shape)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def reconstruct(inp, albedo_guide, gb, fill, ax, ay, cfg=None):
    """-> out_color float32 (h, w, 4).  inp: the input frame (h, w, 4); albedo_guide: the rendered albedo guide; gb: the
    G-buffer dict (prim, position, normal, albedo); fill / ax / ay: writers()."""
    cfg = dict(DEFAULTS, **(cfg or {}))
    C = np.ascontiguousarray(inp, np.float32)
    h, w = fill.shape
    levels, remod = int(cfg["levels"]), int(cfg["remodulate"])
    act = ((fill == 2) & bool(levels & 1)) | ((fill == 4) & bool(levels & 2))
    f = np.where(act, fill, 4)
    s = f32(cfg["support"])
    inv_s = np.where(f == 2, f32(1.0) / (s * f32(2.0)), f32(1.0) / (s * f32(4.0))).astype(np.float32)
    inv_n, inv_z = inv_sq(cfg["normal_sigma"]), inv_sq(cfg["depth_sigma"])
    miss = gb["prim"] == MISS
    N = np.ascontiguousarray(gb["normal"][..., :3], np.float32)
    X = np.ascontiguousarray(gb["position"][..., :3], np.float32)
    t = gb["position"][..., 3]
    tp2 = t * t
    I = C[..., :3] / demod(albedo_guide) if remod else C[..., :3]
    Y, Xc = np.mgrid[0:h, 0:w]
    sw = np.zeros((h, w), np.float32)
    acc = np.zeros((h, w, 3), np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for j in (-1, 0, 1):
            qy = np.clip(ay + j * f, 0, h - 1)
            hy = np.maximum(f32(0.0), f32(1.0) - np.abs(Y - qy).astype(np.float32) * inv_s)
            for i in (-1, 0, 1):
                qx = np.clip(ax + i * f, 0, w - 1)
                hx = np.maximum(f32(0.0), f32(1.0) - np.abs(Xc - qx).astype(np.float32) * inv_s)
                mq = miss[qy, qx]
                wn = _e(_sq(N[qy, qx] - N) * inv_n)
                dz = _dot(N, X[qy, qx] - X)
                wz = _e(((dz * dz) * inv_z) / tp2)
                both = miss & mq
                wn = np.where(miss != mq, f32(0.0), np.where(both, f32(1.0), wn))
                wz = np.where(miss != mq, f32(0.0), np.where(both, f32(1.0), wz))
                wt = ((hx * hy) * wn) * wz
                sw = sw + wt
                acc = acc + I[qy, qx] * wt[..., None]
        done = act & (sw > 0)
        o = acc / np.where(done, sw, f32(1.0))[..., None]
    if remod:
        o = o * demod(gb["albedo"])
    out = C.copy()
    out[..., :3] = np.where(done[..., None], o, C[..., :3])
    out[..., 3] = np.where(done, f32(1.0), C[..., 3])
    return out
