"""fovpt_variance and fovpt_variance_filter without a GPU: the header, the struct mirrors and the defaults; the restatement
(tests/variance_ref.py) against an independent binary64 per-pixel loop and against what the definition implies -- the history
length, the running mean, a depth step, the spatial branch, rejected landings; a constant image, the B3 kernel's variance
factor, a luminance edge, the fall of the noise with every iteration, 0 iterations."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import header_layout
import variance_ref as vr
from fovpathtracing_optixcodelatest_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CAM = dict(eye=(0.0, 0.0, 0.0), U=(0.75, 0.0, 0.0), V=(0.0, 0.42, 0.0), W=(0.0, 0.0, -1.0))      # depth along W: z = -X.z
ENTRY_POINTS = ("fovpt_variance_defaults", "fovpt_variance", "fovpt_variance_buffers", "fovpt_variance_reset",
                "fovpt_variance_filter_defaults", "fovpt_variance_filter", "fovpt_variance_filter_buffers")


@pytest.fixture(scope="module")
def so():
    lib.build()
    return lib.load()


def ulps(a, b):
    """|a - b| in units of b's last place (binary32)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)


def wall(w, h, z=5.0, normal=(0.0, 0.0, 1.0)):
    """A G-buffer of one plane facing the camera at depth z: position (x, y, -z, t = z), normal, white albedo."""
    pos = np.zeros((h, w, 4), np.float32)
    Y, X = np.mgrid[0:h, 0:w]
    pos[..., 0], pos[..., 1], pos[..., 2], pos[..., 3] = X * 0.01, Y * 0.01, -z, z
    nrm = np.zeros((h, w, 4), np.float32)
    nrm[..., :3] = normal
    alb = np.zeros((h, w, 4), np.float32)
    alb[..., :3] = 1.0
    return dict(position=pos, normal=nrm, albedo=alb)


def sky(gb, mask):
    gb["position"][mask] = (0.0, 0.0, 0.0, -1.0)
    gb["normal"][mask] = 0.0
    gb["albedo"][mask] = 0.0
    return gb


def noise(w, h, seed, lo=0.2, hi=1.8):
    c = np.random.default_rng(seed).uniform(lo, hi, (h, w, 4)).astype(np.float32)
    c[..., 3] = 1.0
    return c


# ---- the header and the ABI ---------------------------------------------------------------------------------------------------------
def _args(hdr, name):
    m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
    assert m, "fovpt.h does not declare %s" % name
    return [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", a).strip()) for a in m.group(1).replace("\n", " ").split(",")]


def test_the_header_declares_every_entry_point():
    hdr = open(os.path.join(ROOT, "include", "fovpt.h")).read()
    assert _args(hdr, "fovpt_variance_defaults") == ["fovpt_variance_config* out"]
    assert _args(hdr, "fovpt_variance") == ["fovpt_ctx* ctx", "const fovpt_launch_params* lp", "const fovpt_variance_config* vc",
                                            "const fovpt_gbuffer_ptrs* gbuffer", "const fovpt_float4* in_sample", "const fovpt_float4* motion",
                                            "fovpt_float4* out_variance"]
    assert _args(hdr, "fovpt_variance_buffers") == ["fovpt_ctx* ctx", "fovpt_float4** variance", "const fovpt_float4** moments"]
    assert _args(hdr, "fovpt_variance_reset") == ["fovpt_ctx* ctx"]
    assert _args(hdr, "fovpt_variance_filter_defaults") == ["fovpt_variance_filter_config* out"]
    assert _args(hdr, "fovpt_variance_filter") == ["fovpt_ctx* ctx", "const fovpt_launch_params* lp", "const fovpt_variance_filter_config* fc",
                                                   "const fovpt_gbuffer_ptrs* gbuffer", "const fovpt_float4* in_color", "const fovpt_float4* variance",
                                                   "fovpt_float4* out_color", "uint32_t* out_rgba"]
    assert _args(hdr, "fovpt_variance_filter_buffers") == ["fovpt_ctx* ctx", "fovpt_float4** color", "uint32_t** rgba"]
    for name in ENTRY_POINTS:
        assert name in lib.EXPORTS


def test_the_library_exports_them_and_holds_the_kernels(so):
    names = subprocess.check_output(["nm", "-D", "--defined-only", lib.SO_PATH], text=True)
    for sym in ENTRY_POINTS:
        assert re.search(r"\bT %s\b" % sym, names), sym
        assert getattr(so, sym).restype == C.c_int
    kernels = subprocess.check_output(["strings", lib.SO_PATH], text=True)
    for k in ("k_variance_moments", "k_vfilter_prep", "k_vfilter_step"):
        assert k in kernels, k


def test_the_struct_mirrors_match_the_header():
    for ctype, mirror, size in (("fovpt_variance_config", abi.VarianceConfig, 32), ("fovpt_variance_filter_config", abi.VarianceFilterConfig, 48)):
        names = [f[0] for f in mirror._fields_]
        got = header_layout.layout(ctype, mirror)
        assert got[0] == C.sizeof(mirror) == size
        assert got[1:] == [getattr(mirror, n).offset for n in names]
    hdr = open(os.path.join(ROOT, "include", "fovpt.h")).read()
    for name in ("fovpt_variance_config", "fovpt_variance_filter_config"):
        assert re.search(r"static_assert\(sizeof\(%s\) == " % name, hdr), name


def test_the_defaults_are_the_documented_ones(so):
    d = abi.VarianceConfig()
    C.memset(C.byref(d), 0xff, C.sizeof(d))
    assert so.fovpt_variance_defaults(C.byref(d)) == 0
    assert (d.history_cap, d.spatial_below, d.spatial_radius, list(d._reserved)) == (16, 4, 3, [0] * 3)
    assert (d.depth_tolerance, d.normal_tolerance) == (f32(0.02), f32(0.1))
    assert {k: f32(v) for k, v in d.as_dict().items()} == {k: f32(v) for k, v in vr.MOMENT_DEFAULTS.items()}
    f = abi.VarianceFilterConfig()
    C.memset(C.byref(f), 0xff, C.sizeof(f))
    assert so.fovpt_variance_filter_defaults(C.byref(f)) == 0
    assert (f.iterations_fovea, f.iterations_middle, f.iterations_periphery, f.iterations_uniform, f.demodulate) == (0, 2, 4, 4, 1)
    assert (f.luminance_sigma, f.normal_sigma, f.depth_sigma, list(f._reserved)) == (f32(4.0), f32(0.5), f32(0.05), [0] * 4)
    assert {k: f32(v) for k, v in f.as_dict().items()} == {k: f32(v) for k, v in vr.FILTER_DEFAULTS.items()}
    assert so.fovpt_variance_defaults(None) == -1 and so.fovpt_variance_filter_defaults(None) == -1
    lp, g = abi.LaunchParams(), abi.GBufferPtrs()
    assert so.fovpt_variance(None, C.byref(lp), C.byref(d), C.byref(g), None, None, None) == -1
    assert so.fovpt_variance_filter(None, C.byref(lp), C.byref(f), C.byref(g), None, None, None, None) == -1
    assert so.fovpt_variance_reset(None) == -1


def test_the_dropin_header_compiles():
    src = '#include "SimplePathtracer.h"\nvoid f(SampleRenderer& s, fovpt_float4* a, uint32_t* p) { fovpt_variance_config vc = s.varianceDefaults(); ' \
          's.variance(); s.variance(vc, nullptr, a, a, a); s.varianceReset(); fovpt_float4* v; const fovpt_float4* m; s.varianceBuffers(&v, &m); ' \
          'fovpt_variance_filter_config fc = s.varianceFilterDefaults(); s.varianceFilter(); s.varianceFilter(fc, nullptr, a, a, a, p); ' \
          'fovpt_float4* c; uint32_t* q; s.varianceFilterBuffers(&c, &q); s.downloadVarianceFiltered(p); s.downloadVariance(a); s.variancePost(vc, fc, a); }\n'
    header_layout.syntax_check(src)


# ---- the moment step ----------------------------------------------------------------------------------------------------------------
def moments_f64(prev, sample, gb, cam, fill, motion, cfg):
    """Section 1 of the definition, pixel by pixel in binary64 (Python floats), written apart from variance_ref."""
    h, w = sample.shape[:2]
    U, V, Wv = (np.array(cam[k], np.float64) for k in ("U", "V", "W"))
    row2 = np.cross(U, V) / np.dot(U, np.cross(V, Wv))
    hist, out = np.zeros((h, w, 4)), np.zeros((h, w, 4))
    L = lambda c: 0.2126 * float(c[0]) + 0.7152 * float(c[1]) + 0.0722 * float(c[2])
    for y in range(h):
        for x in range(w):
            l = L(sample[y, x])
            P, N = gb["position"][y, x].astype(np.float64), gb["normal"][y, x, :3].astype(np.float64)
            miss = P[3] < 0
            zp = -1.0 if miss else float(np.dot(row2, P[:3] - np.array(cam["eye"], np.float64)))
            m1 = m2 = nh = 0.0
            if prev is not None:
                mv = (0.0, 0.0, zp, 1.0) if motion is None else [float(v) for v in motion[y, x]]
                px, py, zr = x + mv[0], y + mv[1], mv[2]
                if mv[3] != 0 and -1 <= px < w and -1 <= py < h:
                    x0, y0 = math.floor(px), math.floor(py)
                    fx, fy = px - x0, py - y0
                    sw = s1 = s2 = sn = 0.0
                    for k, wt in enumerate(((1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy)):
                        qx, qy = x0 + (k & 1), y0 + (k >> 1)
                        if not (0 <= qx < w and 0 <= qy < h):
                            continue
                        q = prev[qy, qx].astype(np.float64)
                        if (q[3] < 0) != miss or (not miss and not abs(q[3] - zr) <= cfg["depth_tolerance"] * zr):
                            continue
                        sw, s1, s2, sn = sw + wt, s1 + wt * q[0], s2 + wt * q[1], sn + wt * q[2]
                    if sw >= 1 / 64:
                        m1, m2, nh = s1 / sw, s2 / sw, sn / sw
            n = min(nh + 1, cfg["history_cap"])
            M1, M2 = (l, l * l) if n == 1 else (m1 + (l - m1) / n, m2 + (l * l - m2) / n)
            hist[y, x] = (M1, M2, n, zp)
            if n >= cfg["spatial_below"]:
                mean, var = M1, max(0.0, M2 - M1 * M1)
            else:
                f, R = int(fill[y, x]), cfg["spatial_radius"]
                s0 = s1 = s2 = 0.0
                for j in range(-R, R + 1):
                    for i in range(-R, R + 1):
                        qx, qy = min(max(x + f * i, 0), w - 1), min(max(y + f * j, 0), h - 1)
                        Pq, Nq = gb["position"][qy, qx].astype(np.float64), gb["normal"][qy, qx, :3].astype(np.float64)
                        ok = (i, j) == (0, 0) or ((Pq[3] < 0) == miss and (miss or (
                            float(np.sum((Nq - N) ** 2)) <= cfg["normal_tolerance"] and abs(float(np.dot(N, Pq[:3] - P[:3]))) <= cfg["depth_tolerance"] * P[3])))
                        if ok:
                            lq = L(sample[qy, qx])
                            s0, s1, s2 = s0 + 1, s1 + lq, s2 + lq * lq
                mean = s1 / s0
                var = max(0.0, s2 / s0 - mean * mean)
            out[y, x] = (var / (mean * mean + 1e-8), var, mean, n)
    return hist, out


def small_scene(w, h, seed):
    """A wall with a nearer slab over its right third and a sky row on top; a fill map with all three fills."""
    gb = wall(w, h, 5.0)
    gb["position"][:, 2 * w // 3:, 2], gb["position"][:, 2 * w // 3:, 3] = -3.0, 3.0
    gb["normal"][:, 2 * w // 3:, :3] = (0.6, 0.0, 0.8)
    sky(gb, np.arange(h)[:, None] * np.ones(w, int)[None, :] == 0)
    fill = np.ones((h, w), np.int64)
    fill[:, : w // 3] = 4
    fill[:, w // 3: w // 2] = 2
    rng = np.random.default_rng(seed)
    mv = np.zeros((h, w, 4), np.float32)
    mv[..., :2] = rng.uniform(-1.6, 1.6, (h, w, 2))
    for y in range(h):
        for x in range(w):
            P = gb["position"][y, x]
            mv[y, x, 2] = -1.0 if P[3] < 0 else -P[2] * rng.choice([1.0, 1.0, 1.0, 1.5])
    mv[..., 3] = rng.choice([1.0, 1.0, 1.0, 0.0], (h, w))
    return gb, fill, mv


@pytest.mark.parametrize("size", [(1, 1), (2, 1), (5, 4), (9, 7)], ids=lambda s: "%dx%d" % s)
def test_the_restatement_agrees_with_a_binary64_loop(size):
    w, h = size
    gb, fill, mv = small_scene(w, h, 3)
    seen = dict(spatial=0, temporal=0, depth=0, cls=0, long=0)
    for cfg in (dict(vr.MOMENT_DEFAULTS), dict(vr.MOMENT_DEFAULTS, history_cap=2, spatial_below=2, spatial_radius=1, depth_tolerance=0.1)):
        prev = prev64 = None
        for k in range(4):
            sample = noise(w, h, 10 + k)
            motion = None if k == 1 else mv
            rec = {}
            hist, out = vr.moments(prev, sample, gb, CAM, fill, motion, cfg, rec)
            h64, o64 = moments_f64(prev, sample, gb, CAM, fill, motion, cfg)      # (from the float32 history: one step's difference)
            assert (np.abs(hist - h64) <= 1e-5 * np.abs(h64)).all(), (size, k, "history")
            # var is the difference of two rounded numbers of the second moment's size, mean^2 + var: 1e-5 relative to that size
            # (relative to var itself nothing holds in binary32 where the two cancel); rel is var over mean^2
            second = o64[..., 2] ** 2 + o64[..., 1]
            scale = np.stack([second / (o64[..., 2] ** 2 + 1e-8), second, np.abs(o64[..., 2]), o64[..., 3]], axis=-1)
            # step 6 is a branch on n, and n_h a rounded average of integers: where the two precisions take different sides of
            # spatial_below (both within the tolerance of it) only n itself is compared
            settled = (hist[..., 2] >= cfg["spatial_below"]) == (h64[..., 2] >= cfg["spatial_below"])
            assert (np.abs(out - o64) <= 1e-5 * scale)[settled].all(), (size, k, "variance")
            assert (np.abs(out - o64) <= 1e-5 * scale)[..., 3].all() and (~settled).mean() < 0.1
            seen["spatial"] += int(rec["spatial"].sum()); seen["temporal"] += int((~rec["spatial"]).sum())
            seen["depth"] += int(rec["reject_depth"].sum()); seen["cls"] += int(rec["reject_class"].sum())
            seen["long"] += int((hist[..., 2] >= 2).sum())
            prev = hist
    if size == (9, 7):
        assert all(v > 0 for v in seen.values()), seen


def test_the_history_length_and_the_running_mean():
    w, h, cap, K = 6, 5, 5, 9
    gb = wall(w, h)
    fill = np.ones((h, w), np.int64)
    cfg = dict(vr.MOMENT_DEFAULTS, history_cap=cap)
    prev, ls = None, []
    ema = None
    for k in range(1, K + 1):
        sample = noise(w, h, 100 + k)
        ls.append(vr.lum(sample[..., :3]).astype(np.float64))
        prev, out = vr.moments(prev, sample, gb, CAM, fill, None, cfg)
        n = min(k, cap)
        assert (prev[..., 2] == n).all() and (out[..., 3] == n).all()      # 1, 2, ..., cap, cap, ...
        # every step rounds l - m1, 1 / n, their product and the sum, each by 2^-24 of a value below 2 max|l|: 2^-21 max|l| a step
        bound = k * 2.0 ** -21 * max(float(np.abs(l).max()) for l in ls)
        if k <= cap:
            assert (np.abs(prev[..., 0] - np.mean(ls, axis=0)) <= bound).all(), k      # the mean of the last n = k frames
            ema = np.mean(ls, axis=0)
        else:
            ema = ema + (ls[-1] - ema) / cap                                            # capped: the recurrence in binary64
            assert (np.abs(prev[..., 0] - ema) <= bound).all(), k
        if k >= 4:
            want = np.maximum(0.0, prev[..., 1].astype(np.float64) - prev[..., 0].astype(np.float64) ** 2)
            assert (np.abs(out[..., 1] - want) <= 1e-5).all() and (out[..., 2] == prev[..., 0]).all()


def test_a_depth_step_keeps_the_two_sides_apart():
    w, h = 8, 3
    gb = wall(w, h, 5.0)
    gb["position"][:, 4:, 2], gb["position"][:, 4:, 3] = -2.0, 2.0           # near side: columns 4 ..
    fill = np.ones((h, w), np.int64)
    first = np.zeros((h, w, 4), np.float32)
    first[:, :4, :3], first[:, 4:, :3] = 1.0, 3.0                              # luminance 1 on the far side, 3 on the near side
    prev, _ = vr.moments(None, first, gb, CAM, fill)
    second = np.zeros((h, w, 4), np.float32)
    second[..., :3] = 2.0
    for shift in (-0.5, 0.5):
        mv = np.zeros((h, w, 4), np.float32)
        mv[..., 0], mv[..., 3] = shift, 1.0
        mv[..., 2] = -gb["position"][..., 2]                                   # the reprojected depth: the pixel's own
        rec = {}
        hist, _ = vr.moments(prev, second, gb, CAM, fill, mv, None, rec)
        x = 4 if shift < 0 else 3                                              # the pixel whose taps straddle the step
        assert rec["reject_depth"][:, x].min() >= 1
        far, near = hist[:, :4], hist[:, 4:]
        # n = 2 where a tap of the own side remains: M1 = m1 + (l - m1) / 2 with m1 the own side's 1 or 3 exactly
        assert (far[..., 0][far[..., 2] == 2] == 1.5).all() and (near[..., 0][near[..., 2] == 2] == 2.5).all()
        assert (hist[:, x, 2] == 2).all() and (hist[..., 2] >= 1).all()
    # with a tolerance that admits the step the two sides mix
    hist, _ = vr.moments(prev, second, gb, CAM, fill, mv, dict(depth_tolerance=1.0))
    assert hist[0, 3, 0] not in (1.5, 2.5)


def test_spatial_below_chooses_the_branch():
    w, h = 7, 6
    gb, fill, mv = small_scene(w, h, 5)
    for below, always in ((0, False), (3, True)):
        cfg = dict(vr.MOMENT_DEFAULTS, history_cap=2, spatial_below=below)      # cap + 1: n never reaches it
        prev = None
        for k in range(3):
            rec = {}
            prev, _ = vr.moments(prev, noise(w, h, k), gb, CAM, fill, None, cfg, rec)
            assert rec["spatial"].all() if always else not rec["spatial"].any()


def test_rejected_landings_start_a_new_history():
    w, h = 6, 4
    gb = wall(w, h)
    fill = np.ones((h, w), np.int64)
    prev, _ = vr.moments(None, noise(w, h, 1), gb, CAM, fill)
    mv = np.zeros((h, w, 4), np.float32)
    mv[..., 2], mv[..., 3] = 5.0, 1.0
    mv[0, 0, 3] = 0.0                                       # w == 0
    mv[0, 1, 0] = np.nan                                    # a NaN
    mv[0, 2, 1] = np.nan
    mv[1, 0, 0] = -1.5                                      # px = -1.5: outside
    mv[1, 5, 0] = 1.0                                       # px = w: outside
    mv[3, 3, 1] = 1.0                                       # py = h: outside
    mv[2, 2, 2] = 9.0                                       # another depth: every tap rejected
    mv[0, 5, 0] = 0.75                                      # px = w - 0.25: inside, one tap column beyond the frame
    hist, out = vr.moments(prev, noise(w, h, 2), gb, CAM, fill, mv)
    new = np.zeros((h, w), bool)
    for y, x in ((0, 0), (0, 1), (0, 2), (1, 0), (1, 5), (3, 3), (2, 2)):
        new[y, x] = True
    assert (hist[..., 2][new] == 1).all() and (hist[..., 2][~new] == 2).all()
    assert np.array_equal(hist[..., 0][new], vr.lum(noise(w, h, 2)[..., :3])[new])


# ---- the filter ---------------------------------------------------------------------------------------------------------------------
def uniform_n(w, h, n):
    return np.ones((h, w), np.int64), np.full((h, w), n, np.int32)


def test_a_constant_image_stays_constant():
    w, h = 23, 19
    gb = wall(w, h)
    color = np.zeros((h, w, 4), np.float32)
    color[..., :3] = (0.37, 1.21, 0.05)
    var = noise(w, h, 4, 0.0, 2.0)
    # the 2 ulp are one weighted average's (acc / sw rounds); an iteration averages the one before it, so k of them stay within 2 k
    for its in (1, 4):
        for fill in (1, 2, 4):
            f, n = uniform_n(w, h, its)
            out, _ = vr.vfilter(color, var, gb, f * fill, n, dict(demodulate=0))
            assert ulps(out[..., :3], color[..., :3]).max() <= 2 * its, (its, fill)
            assert (out[..., 3] == 1).all()


def test_one_iteration_scales_a_constant_variance_by_the_b3_factor():
    w, h, v0 = 21, 17, 0.3
    gb = wall(w, h)
    color = np.ones((h, w, 4), np.float32)                 # luminance 1 (to rounding): v = rel * lum^2
    var = np.full((h, w, 4), v0, np.float32)
    for fill in (1, 2, 4):
        f, n = uniform_n(w, h, 1)
        _, J = vr.vfilter(color, var, gb, f * fill, n, dict(demodulate=0))
        lI = vr.lum(color[..., :3])
        vin = (var[..., 0] * (lI * lI)).astype(np.float64)
        s = 2 * fill
        inner = J[s:h - s, s:w - s, 3].astype(np.float64)
        want = vin[s:h - s, s:w - s] * (35.0 / 128.0) ** 2          # (sum H^2)^2, H = (1, 4, 6, 4, 1) / 16: 70 / 256 a side
        assert inner.size > 0 and (np.abs(inner - want) <= 32 * 2.0 ** -24 * want).all()      # 25 products and sums, one quotient


def test_a_luminance_edge_survives_zero_variance():
    w, h = 24, 12
    gb = wall(w, h)
    color = np.zeros((h, w, 4), np.float32)
    color[:, :12, :3], color[:, 12:, :3] = (0.4, 0.5, 0.3), (1.3, 0.9, 1.7)
    var = np.zeros((h, w, 4), np.float32)
    f, n = uniform_n(w, h, 4)
    rec = []
    out, _ = vr.vfilter(color, var, gb, f, n, dict(demodulate=0), rec)
    assert ulps(out[..., :3], color[..., :3]).max() <= 2
    assert any((wl == 0).any() for _, _, wl in rec)


def test_the_noise_falls_with_every_iteration():
    w, h = 48, 40
    gb = wall(w, h)
    color = noise(w, h, 9, 0.5, 1.5)
    var = np.full((h, w, 4), 4.0, np.float32)              # a large relative variance: the luminance stop is wide open
    last = float(np.var(vr.lum(color[..., :3]).astype(np.float64)))
    for its in (1, 2, 3, 4):
        f, n = uniform_n(w, h, its)
        out, _ = vr.vfilter(color, var, gb, f, n, dict(demodulate=0))
        now = float(np.var(vr.lum(out[..., :3]).astype(np.float64)))
        assert now < last, (its, now, last)
        last = now


def test_no_iterations_return_the_input():
    w, h = 9, 7
    gb, fill, _ = small_scene(w, h, 1)
    color = noise(w, h, 2)
    out, _ = vr.vfilter(color, noise(w, h, 3), gb, fill, np.zeros((h, w), np.int32))
    assert np.array_equal(out[..., :3].view(np.uint32), color[..., :3].view(np.uint32)) and (out[..., 3] == 1).all()
    # and a mix: only the pixels with iterations change
    n = (fill > 1).astype(np.int32) * 2
    out, _ = vr.vfilter(color, noise(w, h, 3), gb, fill, n)
    assert np.array_equal(out[..., :3][n == 0].view(np.uint32), color[..., :3][n == 0].view(np.uint32))
    assert (out[..., :3][n > 0] != color[..., :3][n > 0]).any()
