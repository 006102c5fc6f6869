"""numpy float32 restatement of fovpt_variance and fovpt_variance_filter (csrc/variance.hip): the definition the GPU kernels match
bit for bit.

Every operation below is one IEEE binary32 operation in the order the kernels perform it (the library is built with
-ffp-contract=off, so the device does not fuse any of them either); beyond +, -, * and / there are only floor, min, max and
comparisons.  max is fmax: max(0, NaN) is 0.

    lum(c)  (0.2126 c.x + 0.7152 c.y) + 0.0722 c.z;  sq3(a) = (a.x a.x + a.y a.y) + a.z a.z, dot likewise;  e(d) = max(0, 1 - d)^2
    fill    of a pixel's last writer among the frame's passes (denoise_ref.level_map), 1 where no pass writes

moments(state, sample, gbuffer, cam, motion, cfg) -- one step of the history; the history records are (M1, M2, n, z):
    1  l = lum(sample), l2 = l * l
    2  miss iff position.w < 0;  hit: v = X - eye, z_p = (M[2].x v.x + M[2].y v.y) + M[2].z v.z, M the float32 rows of
       inverse(U V W) (temporal_ref.camera_inverse: binary64, each entry rounded);  miss: z_p = -1
    3  mv = motion or (0, 0, z_p, 1);  no history if mv.w == 0;  px = float(x) + mv.x, py likewise, zr = mv.z;  no history unless
       px >= -1 and px < w and py >= -1 and py < h
    4  x0 = floor(px), fx = px - x0 (y likewise); taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) with weights
       (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy; a tap inside the frame is kept iff (z_q < 0) is the pixel's class and, for
       hits, |z_q - zr| <= depth_tolerance * zr;  sw = sum of kept w;  sw >= 1/64: m1 = (sum M1_q w) / sw, m2, n_h likewise; else n_h = 0
    5  n = min(n_h + 1, cap);  n == 1: M1 = l, M2 = l2;  else M1 = m1 + (1 / n)(l - m1), M2 = m2 + (1 / n)(l2 - m2)
    6  n >= spatial_below: mean = M1, var = max(0, M2 - M1 M1);  else over taps q = clamp(p + fill (i, j)), j (rows) outer, i inner,
       -R .. R: w = 1 for the centre, and for another tap iff same class and, for hits, sq3(N_q - N_p) <= normal_tolerance and
       |dot(N_p, X_q - X_p)| <= depth_tolerance * t_p;  s0 += w, s1 += w l_q, s2 += w (l_q l_q);  mean = s1 / s0,
       var = max(0, s2 / s0 - mean mean)
    7  out = (var / (mean mean + 1e-8), var, mean, n)

vfilter(color, variance, gbuffer, fill, n, cfg):
    prep   D = demodulate ? demod(albedo) : 1 (demod: denoise_ref's D);  I = C / D;  v = variance.x * (lum(I) lum(I))
    iteration i < n (the other pixels keep (I, v)), s = fill 2^i:
       g = sum G_ij v(clamp(p + fill (i, j))), j outer, G = (1/4, 1/8, 1/16 by the number of non-zero offsets)
       kl = 1 / ((sigma_l sigma_l) g + 1e-6)
       taps q = clamp(p + s (dx, dy)), dy outer:  d = lum(I_q) - lum(I_p), wl = e((d d) kl);  class mismatch: wn = wz = 0;  two
       misses: 1;  two hits: wn = e(sq3(N_q - N_p) inv_n), wz = e(((dz dz) inv_z) / (t_p t_p)), dz = dot(N_p, X_q - X_p)
       wt = (((H_dx H_dy) wl) wn) wz;  sw += wt, acc += I_q wt, sv += (wt wt) v_q;  I' = acc / sw, v' = sv / (sw sw)
    output n >= 1: I * D, else C; alpha 1.  rgba8 = make_color(reinhard(out * 16, 1)) (the resolve's tone map)"""
import numpy as np

import denoise_ref as dn
import temporal_ref as tr

f32 = np.float32
H = dn.H
MOMENT_DEFAULTS = dict(history_cap=16, spatial_below=4, spatial_radius=3, depth_tolerance=0.02, normal_tolerance=0.1)
FILTER_DEFAULTS = dict(iterations_fovea=0, iterations_middle=2, iterations_periphery=4, iterations_uniform=4,
                       luminance_sigma=4.0, normal_sigma=0.5, depth_sigma=0.05, demodulate=1)


def lum(v):
    return (f32(0.2126) * v[..., 0] + f32(0.7152) * v[..., 1]) + f32(0.0722) * v[..., 2]


def sq3(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def edge(d):
    t = np.fmax(f32(0.0), f32(1.0) - d)
    return t * t


def fills(w, h, gaze, r_inner, r_outer, uniform):
    """-> (fill per pixel with 1 where no pass writes, pass per pixel with -1 there)."""
    fill, pas = dn.level_map(w, h, gaze, r_inner, r_outer, uniform)
    return np.where(pas < 0, 1, fill).astype(np.int64), pas


def depth_row(cam):
    """M[2]: the third row of the float32 inverse(U V W), or None for a singular camera."""
    M = tr.camera_inverse(cam["U"], cam["V"], cam["W"])
    return None if M is None else M[2].astype(np.float32)


def moments(prev, sample, gb, cam, fill, motion=None, cfg=None, record=None):
    """One step.  prev: the previous history (h, w, 4) float32 or None (no history); sample (h, w, 4); gb: dict with position and
    normal (h, w, 4); cam: dict eye, U, V, W; fill (h, w) int; motion (h, w, 4) or None.  -> (history, variance image), both
    (h, w, 4) float32.  record: a dict that receives reject_depth, reject_class (taps of step 4 inside the frame, per pixel),
    spatial (h, w) bool: step 6 took the window."""
    cfg = dict(MOMENT_DEFAULTS, **(cfg or {}))
    S = np.ascontiguousarray(sample, np.float32)
    P = np.ascontiguousarray(gb["position"], np.float32)
    N = np.ascontiguousarray(gb["normal"], np.float32)[..., :3]
    h, w = S.shape[:2]
    ztol_c, ntol = f32(cfg["depth_tolerance"]), f32(cfg["normal_tolerance"])
    cap, below, R = int(cfg["history_cap"]), int(cfg["spatial_below"]), int(cfg["spatial_radius"])
    Y, X = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        l = lum(S)
        l2 = l * l
        miss = P[..., 3] < 0
        eye = np.asarray(cam["eye"], np.float32)
        m = depth_row(cam)
        v = P[..., :3] - eye
        zp = np.where(miss, f32(-1.0), (m[0] * v[..., 0] + m[1] * v[..., 1]) + m[2] * v[..., 2]).astype(np.float32)
        m1 = np.zeros((h, w), np.float32)
        m2 = np.zeros((h, w), np.float32)
        nh = np.zeros((h, w), np.float32)
        rej_depth = np.zeros((h, w), np.int32)
        rej_class = np.zeros((h, w), np.int32)
        if prev is not None:
            if motion is None:
                mv = np.zeros((h, w, 4), np.float32)
                mv[..., 2], mv[..., 3] = zp, 1.0
            else:
                mv = np.ascontiguousarray(motion, np.float32)
            px = X.astype(np.float32) + mv[..., 0]
            py = Y.astype(np.float32) + mv[..., 1]
            zr = mv[..., 2]
            ok = ~(mv[..., 3] == 0) & (px >= f32(-1.0)) & (px < f32(w)) & (py >= f32(-1.0)) & (py < f32(h))
            pxs, pys = np.where(ok, px, f32(0.0)), np.where(ok, py, f32(0.0))
            x0f, y0f = np.floor(pxs), np.floor(pys)
            fx, fy = pxs - x0f, pys - y0f
            x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
            one = f32(1.0)
            wts = ((one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy)
            ztol = ztol_c * zr
            sw = np.zeros((h, w), np.float32)
            s1, s2, sn = sw.copy(), sw.copy(), sw.copy()
            for k in range(4):
                qx, qy = x0 + (k & 1), y0 + (k >> 1)
                inside = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                hq = prev[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)]
                same = (hq[..., 3] < 0) == miss
                near = miss | (np.abs(hq[..., 3] - zr) <= ztol)
                keep = inside & same & near
                rej_class += inside & ~same
                rej_depth += inside & same & ~near
                sw = np.where(keep, sw + wts[k], sw)
                s1 = np.where(keep, s1 + hq[..., 0] * wts[k], s1)
                s2 = np.where(keep, s2 + hq[..., 1] * wts[k], s2)
                sn = np.where(keep, sn + hq[..., 2] * wts[k], sn)
            has = ok & (sw >= f32(1.0 / 64))
            den = np.where(has, sw, one)
            m1 = np.where(has, s1 / den, f32(0.0))
            m2 = np.where(has, s2 / den, f32(0.0))
            nh = np.where(has, sn / den, f32(0.0))
        n = np.fmin(nh + f32(1.0), f32(cap))
        t = f32(1.0) / n
        first = n == 1
        M1 = np.where(first, l, m1 + t * (l - m1))
        M2 = np.where(first, l2, m2 + t * (l2 - m2))
        hist = np.stack([M1, M2, n, zp], axis=-1).astype(np.float32)
        mean = M1
        var = np.fmax(f32(0.0), M2 - M1 * M1)
        spatial = ~(n >= f32(below))
        if spatial.any():
            s0 = np.zeros((h, w), np.float32)
            s1, s2 = s0.copy(), s0.copy()
            ztol = ztol_c * P[..., 3]
            for j in range(-R, R + 1):
                qy = np.clip(Y + fill * j, 0, h - 1)
                for i in range(-R, R + 1):
                    qx = np.clip(X + fill * i, 0, w - 1)
                    Pq, Nq, lq = P[qy, qx], N[qy, qx], l[qy, qx]
                    if i == 0 and j == 0:
                        wq = np.ones((h, w), np.float32)
                    else:
                        same = (Pq[..., 3] < 0) == miss
                        geo = (sq3(Nq - N) <= ntol) & (np.abs(dot(N, Pq[..., :3] - P[..., :3])) <= ztol)
                        wq = np.where(same & (miss | geo), f32(1.0), f32(0.0))
                    s0 = s0 + wq
                    s1 = s1 + wq * lq
                    s2 = s2 + wq * (lq * lq)
            smean = s1 / s0
            svar = np.fmax(f32(0.0), s2 / s0 - smean * smean)
            mean = np.where(spatial, smean, mean)
            var = np.where(spatial, svar, var)
        rel = var / (mean * mean + f32(1e-8))
        out = np.stack([rel, var, mean, n], axis=-1).astype(np.float32)
    if record is not None:
        record.update(reject_depth=rej_depth, reject_class=rej_class, spatial=spatial)
    return hist, out


def iteration_map(fill, pas, cfg, uniform):
    """Iterations per pixel, as the denoiser's: by the pass of the last writer, 0 where no pass writes."""
    return dn.iteration_map(fill, pas, dict(FILTER_DEFAULTS, **(cfg or {})), uniform)


def vfilter(color, variance, gb, fill, n, cfg=None, record=None):
    """-> (out_color (h, w, 4) float32, J = (I, v) after the last iteration (h, w, 4)).  color (h, w, 4); variance (h, w, 4): .x is
    read; gb: dict position, normal and (with demodulate) albedo; fill, n (h, w) int.  record: a list that receives every tap's
    (i, active, wl)."""
    cfg = dict(FILTER_DEFAULTS, **(cfg or {}))
    C = np.ascontiguousarray(color, np.float32)[..., :3]
    P = np.ascontiguousarray(gb["position"], np.float32)
    N = np.ascontiguousarray(gb["normal"], np.float32)[..., :3]
    h, w = C.shape[:2]
    sl = f32(cfg["luminance_sigma"])
    sl2, inv_n, inv_z = sl * sl, dn.inv_sq(cfg["normal_sigma"]), dn.inv_sq(cfg["depth_sigma"])
    Y, X = np.mgrid[0:h, 0:w]
    fill = np.asarray(fill, np.int64)
    with np.errstate(all="ignore"):
        if cfg["demodulate"]:
            A = np.ascontiguousarray(gb["albedo"], np.float32)[..., :3]
            asum = (A[..., 0] + A[..., 1]) + A[..., 2]
            D = np.where((asum > 0)[..., None], np.fmax(A, f32(1.0 / 64)), f32(1.0)).astype(np.float32)
        else:
            D = np.ones((h, w, 3), np.float32)
        I = C / D
        lI = lum(I)
        v = np.ascontiguousarray(variance, np.float32)[..., 0] * (lI * lI)
        miss = P[..., 3] < 0
        tp2 = P[..., 3] * P[..., 3]
        nmax = int(n.max()) if n.size else 0
        for it in range(nmax):
            act = it < n
            s = fill << it
            g = np.zeros((h, w), np.float32)
            for j in (-1, 0, 1):
                qy = np.clip(Y + fill * j, 0, h - 1)
                for i in (-1, 0, 1):
                    qx = np.clip(X + fill * i, 0, w - 1)
                    G = f32((0.5 if i == 0 else 0.25) * (0.5 if j == 0 else 0.25))
                    g = g + G * v[qy, qx]
            kl = f32(1.0) / (sl2 * g + f32(1e-6))
            lp = lum(I)
            sw = np.zeros((h, w), np.float32)
            sv = np.zeros((h, w), np.float32)
            acc = np.zeros((h, w, 3), np.float32)
            for dy in range(-2, 3):
                qy = np.clip(Y + s * dy, 0, h - 1)
                for dx in range(-2, 3):
                    qx = np.clip(X + s * dx, 0, w - 1)
                    Iq, Pq, Nq, vq = I[qy, qx], P[qy, qx], N[qy, qx], v[qy, qx]
                    d = lum(Iq) - lp
                    wl = edge((d * d) * kl)
                    miss_q = Pq[..., 3] < 0
                    wn_h = edge(sq3(Nq - N) * inv_n)
                    dz = dot(N, Pq[..., :3] - P[..., :3])
                    wz_h = edge(((dz * dz) * inv_z) / tp2)
                    wn = np.where(miss != miss_q, f32(0.0), np.where(miss, f32(1.0), wn_h))
                    wz = np.where(miss != miss_q, f32(0.0), np.where(miss, f32(1.0), wz_h))
                    wt = (((H[dx + 2] * H[dy + 2]) * wl) * wn) * wz
                    sw = sw + wt
                    acc = acc + Iq * wt[..., None]
                    sv = sv + (wt * wt) * vq
                    if record is not None:
                        record.append((it, act, wl))
            den = np.where(act, sw, f32(1.0))
            I = np.where(act[..., None], acc / den[..., None], I)
            v = np.where(act, sv / (den * den), v)
        out = np.empty((h, w, 4), np.float32)
        out[..., :3] = np.where((n >= 1)[..., None], I * D, C)
        out[..., 3] = 1.0
    return out, np.concatenate([I, v[..., None]], axis=-1).astype(np.float32)
