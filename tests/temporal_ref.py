"""numpy float32 restatement of fovpt_temporal (csrc/temporal.hip): the definition the GPU kernel matches bit for bit.

Every operation below is one IEEE binary32 operation in the order the kernel performs it (the library is built with
-ffp-contract=off, so the device does not fuse any of them either); the previous camera's inverse is binary64 on the host,
each entry rounded to binary32.

    cap     the fill of the pixel's last writer (reconstruct_ref.writers): 4 -> history_periphery, 2 -> history_middle,
            1 -> history_fovea; a FOV_OFF frame: history_uniform; no writer: 1
    M       rows of [U V W]^-1 of the previous camera: (V x W) / det, (W x U) / det, (U x V) / det, det = U . (V x W)
            (binary64; det 0 or not finite: no pixel reprojects)
    v       hit: X_p - eye_prev; miss: (dx U + dy V) + W, the G-buffer ray of the pixel before normalising (current camera)
    a_k     (M_k.x v.x + M_k.y v.y) + M_k.z v.z
    p       a.z > 0 and -1 <= px < w, -1 <= py < h, px = (((a.x / a.z) + 1) * 0.5) * w - 0.5 (py likewise)
    taps    x0 = floor(px), y0 = floor(py), fx = px - x0, fy = py - y0; (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) with
            weights (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy; a tap is kept if it is in the frame, of p's class (both misses
            or both hits) and for hits sq3(N_q - N_p) <= normal_tolerance and |N_p . (X_q - X_p)| <= depth_tolerance * t_p
            (the previous G-buffer's N_q, X_q)
    sums    in tap order: sw += w, acc += H_q w, sn += n_q w; sw >= 1/64: H = acc / sw, n_h = sn / sw; else n_h = 0
    blend   n = fmin(n_h + 1, cap); n == 1: out = in (all four components, bit for bit), history (in.rgb, 1);
            else out = H + (1 / n) (in - H), alpha 1, history (out, n)
    rgba8   make_color(reinhard(out * 16, 1)) for every pixel (the resolve's tone map)"""
import numpy as np

f32 = np.float32
DEFAULTS = dict(history_fovea=1, history_middle=4, history_periphery=8, history_uniform=4, normal_tolerance=0.1,
                depth_tolerance=0.02)
MAX_HISTORY = 64
MISS = np.uint32(0xffffffff)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _sq(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def caps(fill, uniform, cfg=None):
    """Per-pixel history cap (int64) from the writer fill map (0: no writer) of a frame rendered FOV_OFF (uniform) or not."""
    cfg = dict(DEFAULTS, **(cfg or {}))
    if uniform:
        by = np.full(fill.shape, cfg["history_uniform"], np.int64)
    else:
        by = np.where(fill == 4, cfg["history_periphery"], np.where(fill == 2, cfg["history_middle"], cfg["history_fovea"]))
    return np.where(fill > 0, by, 1).astype(np.int64)


def camera_inverse(U, V, W):
    """Rows of [U V W]^-1 (U, V, W its columns) as the host computes them -> (3, 3) float32, or None when det is 0 or not
    finite.  Cross products (a.y b.z - a.z b.y, ...), dot products (x + y) + z, all in binary64."""
    u, v, w = (tuple(float(f32(c)) for c in x) for x in (U, V, W))

    def cross(a, b):
        return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])

    rows = (cross(v, w), cross(w, u), cross(u, v))
    det = (u[0] * rows[0][0] + u[1] * rows[0][1]) + u[2] * rows[0][2]
    if det == 0.0 or not np.isfinite(det):
        return None
    return np.array([[r[j] / det for j in range(3)] for r in rows], np.float64).astype(np.float32)


def miss_dirs(w, h, U, V, W):
    """(h, w, 3): dx U + dy V + W of the G-buffer's rays (generate_rays' expression with jitter 0.5), not normalised."""
    y, x = np.mgrid[0:h, 0:w]
    dx = f32(2.0) * ((x.astype(np.float32) + f32(0.5)) / f32(w)) - f32(1.0)
    dy = f32(2.0) * ((y.astype(np.float32) + f32(0.5)) / f32(h)) - f32(1.0)
    U, V, W = (np.asarray(v, np.float32) for v in (U, V, W))
    return (dx[..., None] * U + dy[..., None] * V) + W


def project(gb, cam, prev_cam, M=None):
    """-> (px, py, ok) float32 / bool (h, w): where each pixel of the G-buffer gb (seen by cam) lies in prev_cam's frame, and
    whether it reprojects (a.z > 0, -1 <= px < w, -1 <= py < h).  M: camera_inverse(prev_cam) (None: computed here; a singular
    camera reprojects nothing)."""
    h, w = gb["prim"].shape
    M = M if M is not None else camera_inverse(prev_cam["U"], prev_cam["V"], prev_cam["W"])
    if M is None:
        z = np.zeros((h, w), np.float32)
        return z, z.copy(), np.zeros((h, w), bool)
    miss = gb["prim"] == MISS
    X = np.ascontiguousarray(gb["position"][..., :3], np.float32)
    v = np.where(miss[..., None], miss_dirs(w, h, cam["U"], cam["V"], cam["W"]), X - np.asarray(prev_cam["eye"], np.float32))
    a = [(M[k, 0] * v[..., 0] + M[k, 1] * v[..., 1]) + M[k, 2] * v[..., 2] for k in range(3)]
    fw, fh = f32(w), f32(h)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        px = (((a[0] / a[2]) + f32(1.0)) * f32(0.5)) * fw - f32(0.5)
        py = (((a[1] / a[2]) + f32(1.0)) * f32(0.5)) * fh - f32(0.5)
        ok = (a[2] > 0) & (px >= -1) & (px < fw) & (py >= -1) & (py < fh)
    return px.astype(np.float32), py.astype(np.float32), ok


def step(inp, gb, cap, cam, prev=None, cfg=None):
    """One step -> (out_color (h, w, 4) float32, history (h, w, 4) float32).

    inp: the input frame (h, w, 4); gb: the G-buffer of the frame's camera (dict prim, position, normal as fovpt_gbuffer);
    cap: caps(); cam: the frame's camera, dict eye / U / V / W; prev: None (no history) or dict(gb=, cam=, history=) of the
    previous step."""
    cfg = dict(DEFAULTS, **(cfg or {}))
    C = np.ascontiguousarray(inp, np.float32)
    h, w = cap.shape
    nh = np.zeros((h, w), np.float32)
    H = np.zeros((h, w, 3), np.float32)
    M = None
    if prev is not None and prev["history"].shape[:2] == (h, w):
        M = camera_inverse(prev["cam"]["U"], prev["cam"]["V"], prev["cam"]["W"])
    if M is not None:
        miss = gb["prim"] == MISS
        X = np.ascontiguousarray(gb["position"][..., :3], np.float32)
        t = gb["position"][..., 3]
        N = np.ascontiguousarray(gb["normal"][..., :3], np.float32)
        px, py, ok = project(gb, cam, prev["cam"], M)
        ok &= cap > 1
        with np.errstate(invalid="ignore", over="ignore"):
            px, py = np.where(ok, px, f32(0.0)), np.where(ok, py, f32(0.0))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            x0f, y0f = np.floor(px), np.floor(py)
            fx, fy = px - x0f, py - y0f
            x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
            one = f32(1.0)
            wts = ((one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy)
            pg, ph = prev["gb"], np.ascontiguousarray(prev["history"], np.float32)
            pmiss = pg["prim"] == MISS
            PX = np.ascontiguousarray(pg["position"][..., :3], np.float32)
            PN = np.ascontiguousarray(pg["normal"][..., :3], np.float32)
            ztol = f32(cfg["depth_tolerance"]) * t
            ntol = f32(cfg["normal_tolerance"])
            sw = np.zeros((h, w), np.float32)
            sn = np.zeros((h, w), np.float32)
            acc = np.zeros((h, w, 3), np.float32)
            for k in range(4):
                qx, qy = x0 + (k & 1), y0 + (k >> 1)
                inb = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                keep = inb & (pmiss[cy, cx] == miss)
                nt = _sq(PN[cy, cx] - N) <= ntol
                zt = np.abs(_dot(N, PX[cy, cx] - X)) <= ztol
                keep &= miss | (nt & zt)
                wk = wts[k]
                hq = ph[cy, cx]
                sw = np.where(keep, sw + wk, sw)
                acc = np.where(keep[..., None], acc + hq[..., :3] * wk[..., None], acc)
                sn = np.where(keep, sn + hq[..., 3] * wk, sn)
            got = ok & (sw >= f32(1.0 / 64.0))
            H = np.where(got[..., None], acc / sw[..., None], f32(0.0)).astype(np.float32)
            nh = np.where(got, sn / sw, f32(0.0)).astype(np.float32)
    n = np.fmin(nh + f32(1.0), cap.astype(np.float32))
    same = n == f32(1.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        o = H + (f32(1.0) / n)[..., None] * (C[..., :3] - H)
    out = np.empty_like(C)
    out[..., :3] = np.where(same[..., None], C[..., :3], o)
    out[..., 3] = np.where(same, C[..., 3], f32(1.0))
    hist = np.empty_like(C)
    hist[..., :3] = out[..., :3]
    hist[..., 3] = np.where(same, f32(1.0), n)
    return out, hist
