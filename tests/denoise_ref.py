"""numpy float32 restatement of fovpt_denoise (csrc/denoise.hip): the definition the GPU kernels match bit for bit.

Every operation below is one IEEE binary32 operation in the order the kernels perform it (the library is built with
-ffp-contract=off, so the device does not fuse any of them either).

    level   each pixel's last writer among the frame's passes (P, M, F in that order, or the one FOV_OFF pass): its fill
            f (4, 2, 1) and iteration count n from the config; no writer -> n = 0
    D       (A.x + A.y + A.z > 0) ? max(A, 1/64) : (1, 1, 1)          albedo demodulation, A = albedo guide
    I       C / D                                                   C = color guide (= accum_buffer)
    iteration i = 0 .. max(n) - 1, for pixels with i < n (the others keep I):
            s = f * 2^i; taps q = clamp(p + s * (dx, dy)) for dy in -2..2 (outer), dx in -2..2 (inner)
            h = H[dx] * H[dy], H = (1/16, 1/4, 3/8, 1/4, 1/16)
            e(d) = max(0, 1 - d)^2
            w_c = e(|I_q - I_p|^2 * k),  k = (inv_c * 4^i) / (1e-4 + lum(I_p)^2)
            w_n = 1 if N_p and N_q are both zero, 0 if one is, else e(|N_q - N_p|^2 * inv_n)
            w_a = e(|A_q - A_p|^2 * inv_a)
            w = ((h * w_c) * w_n) * w_a;  I'_p = (sum w * I_q) / (sum w), sums in tap order
    output  n >= 1: I * D, else C; alpha 1.  rgba8 = make_color(reinhard(out * 16, 1)) (the resolve's tone map)

inv_c, inv_n, inv_a = 1 / sigma^2 are computed once in float32 (the library does the same on the host)."""
import numpy as np

f32 = np.float32
H = np.array([1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16], np.float32)   # exact in binary32
DEFAULTS = dict(iterations_fovea=0, iterations_middle=2, iterations_periphery=3, iterations_uniform=3,
                color_sigma=8.0, normal_sigma=0.5, albedo_sigma=0.2)


def inv_sq(sigma):
    s = f32(sigma)
    return f32(1.0) / (s * s)


def _e(d):
    t = np.maximum(f32(0.0), f32(1.0) - d)
    return t * t


def _lum(v):
    return (f32(0.2126) * v[..., 0] + f32(0.7152) * v[..., 1]) + f32(0.0722) * v[..., 2]


def _sq(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def frame_passes(w, h, gaze, r_inner, r_outer, uniform):
    """The passes fovpt_render runs (frame_passes in fovpt_api.hip, SimplePathtracer.cpp:85-209):
    (grid w, grid h, factor, fill, offset x, offset y, ring r_inner, ring r_outer) in launch order; offsets wrap as uint32."""
    if uniform:
        return [(w, h, 1, 1, 0, 0, 0.0, 1e9)]
    cx, cy = gaze
    m, f = r_outer + 2, r_inner + 1
    u32 = lambda v: v & 0xffffffff
    return [(w // 4, h // 4, 4, 4, 0, 0, float(r_outer), 1e9),
            (m, m, 2, 2, u32(cx - m), u32(cy - m), float(r_inner), float(m)),
            (2 * f, 2 * f, 1, 1, u32(cx - f), u32(cy - f), 0.0, float(f))]


def level_map(w, h, gaze, r_inner, r_outer, uniform):
    """(fill, pass) per pixel of the last writer: every launch index that passes the ring test (on its block's top-left
    pixel, deviceProgram.cu:433-440) writes its fill x fill block, clamped onto the frame's last row / column (:546-554);
    later passes overwrite earlier ones.  The block's pixel indices are uint32 sums like the launch's (deviceProgram.cu:546-554):
    a launch at a wrapped index 0xffffffff writes pixel 0 and the last row / column.  fill 0 / pass -1: no writer."""
    fill = np.zeros((h, w), np.int32)
    pas = np.full((h, w), -1, np.int32)
    cx, cy = gaze
    for p, (gw, gh, fac, fl, ox, oy, r_in, r_out) in enumerate(frame_passes(w, h, gaze, r_inner, r_outer, uniform)):
        ly, lx = np.mgrid[0:gh, 0:gw].astype(np.uint64)
        ix = (lx * fac + ox) & 0xffffffff
        iy = (ly * fac + oy) & 0xffffffff
        dx = ix.astype(np.float32) - f32(cx)
        dy = iy.astype(np.float32) - f32(cy)
        rng = np.sqrt((dx * dx + dy * dy) + f32(0.0))
        alive = ~((rng < f32(r_in)) | (rng > f32(r_out)))
        ix, iy = ix[alive], iy[alive]
        for v in range(fl):
            for u in range(fl):
                px = np.minimum((ix + u) & 0xffffffff, w - 1).astype(np.int64)      # uint32 sums: 0xffffffff + 1 is pixel 0
                py = np.minimum((iy + v) & 0xffffffff, h - 1).astype(np.int64)
                fill[py, px] = fl
                pas[py, px] = p
    return fill, pas


def iteration_map(fill, pas, cfg, uniform):
    """Iterations per pixel: by the pass of its last writer (P, M, F), or iterations_uniform in FOV_OFF frames."""
    n = np.zeros(fill.shape, np.int32)
    if uniform:
        n[pas == 0] = cfg["iterations_uniform"]
    else:
        for p, key in enumerate(("iterations_periphery", "iterations_middle", "iterations_fovea")):
            n[pas == p] = cfg[key]
    return n


def denoise(color, normal, albedo, fill, n, cfg, record=None):
    """-> (out_color float32 (h, w, 4), filtered I before remodulation).  color / normal / albedo: the guide buffers.
    record: a list that receives (i, active, w) for every tap of iteration i and then (i, active, sum w)."""
    cfg = dict(DEFAULTS, **cfg)
    C = np.ascontiguousarray(color[..., :3], np.float32)
    N = np.ascontiguousarray(normal[..., :3], np.float32)
    A = np.ascontiguousarray(albedo[..., :3], np.float32)
    h, w = fill.shape
    inv_c, inv_n, inv_a = inv_sq(cfg["color_sigma"]), inv_sq(cfg["normal_sigma"]), inv_sq(cfg["albedo_sigma"])
    asum = (A[..., 0] + A[..., 1]) + A[..., 2]
    D = np.where((asum > 0)[..., None], np.maximum(A, f32(1.0 / 64)), f32(1.0))
    I = C / D
    Nzero = (N[..., 0] == 0) & (N[..., 1] == 0) & (N[..., 2] == 0)
    Y, X = np.mgrid[0:h, 0:w]
    nmax = int(n.max()) if n.size else 0
    for i in range(nmax):
        act = i < n
        s = fill.astype(np.int64) << i
        k = (inv_c * f32(4 ** i)) / (f32(1e-4) + _lum(I) * _lum(I))
        sw = np.zeros((h, w), np.float32)
        acc = np.zeros((h, w, 3), np.float32)
        for dy in range(-2, 3):
            qy = np.clip(Y + s * dy, 0, h - 1)
            for dx in range(-2, 3):
                qx = np.clip(X + s * dx, 0, w - 1)
                Iq, Nq, Aq = I[qy, qx], N[qy, qx], A[qy, qx]
                wc = _e(_sq(Iq - I) * k)
                nq0 = Nzero[qy, qx]
                wn = np.where(Nzero & nq0, f32(1.0), np.where(Nzero | nq0, f32(0.0), _e(_sq(Nq - N) * inv_n)))
                wa = _e(_sq(Aq - A) * inv_a)
                wt = ((H[dx + 2] * H[dy + 2] * wc) * wn) * wa
                sw = sw + wt
                acc = acc + Iq * wt[..., None]
                if record is not None:
                    record.append((i, act, wt))
        if record is not None:
            record.append((i, act, sw))
        I = np.where(act[..., None], acc / np.where(act, sw, f32(1.0))[..., None], I)
    out = np.empty((h, w, 4), np.float32)
    out[..., :3] = np.where((n >= 1)[..., None], I * D, C)
    out[..., 3] = 1.0
    return out, I
