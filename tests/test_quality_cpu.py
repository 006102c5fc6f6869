"""fovpt_quality without a GPU: the restatement tests/quality_ref.py against an independent float64 SSIM and a direct MSE / PSNR, the
host implementation (csrc/quality_host.cpp through the loader library) against the restatement bit for bit on the cases of
tests/quality_cases.py, the score functions on hand-made sums, the host implementation under the sanitizers in a program of its
own, and the ABI."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import header_layout
import quality_cases as qc
import quality_ref as qr
from fovpathtracing_optixcodelatest_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fovpathtracing_optixcodelatest_amd", "csrc")
E_INVALID = -1


@pytest.fixture(scope="module")
def cases():
    return qc.cases()


@pytest.fixture(scope="module")
def loader():
    return lib.load_loader()


# ---- 1. the restatement against independent statements ------------------------------------------------------------------------------
def _float_ssim(T, F, x0, y0):
    """The textbook SSIM of one 8 x 8 window in float64: means, variances, covariance, c1 = (0.01 * 255)^2, c2 = (0.03 * 255)^2."""
    a, b = T[y0:y0 + 8, x0:x0 + 8].astype(np.float64), F[y0:y0 + 8, x0:x0 + 8].astype(np.float64)
    ma, mb = a.mean(), b.mean()
    va, vb, cov = ((a - ma) ** 2).mean(), ((b - mb) ** 2).mean(), ((a - ma) * (b - mb)).mean()
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    return ((2 * ma * mb + c1) * (2 * cov + c2)) / ((ma * ma + mb * mb + c1) * (va + vb + c2))


@pytest.mark.parametrize("kind", ["random", "identical", "black_white", "checker", "smooth"])
def test_the_integer_ssim_is_the_float64_ssim(kind):
    """Per window, to within 2^-20 + 1e-9: half a unit of q's scale (2^-21) for its rounding, the rest for the rounding of C1 and
    C2 to integers (relative 9e-6 and 7e-7) on images where the constants are a small share of both factors: all of these.  (A
    flat, nearly black window, where C1 is most of the first factor's terms, would show C1's rounding at about 2e-6.)  This pins
    the integer formulation; it is no tolerance on the code under test."""
    rng = np.random.default_rng(5)
    w, h = 37, 29
    if kind == "smooth":
        yy, xx = np.mgrid[0:h, 0:w]
        g = (4 * xx + 3 * yy).astype(np.uint32) & 255
        test = g | (g << 8) | (g << 16)
        ref = np.clip(g.astype(np.int64) + rng.integers(-6, 7, (h, w)), 0, 255).astype(np.uint32) * np.uint32(0x010101)
    else:
        test, ref = qc.images_of(kind, w, h, rng)
    T, F = qr.luma(test), qr.luma(ref)
    ys, xs, q = qr.window_q(T, F)
    assert list(xs) == list(range(0, w - 7, 4)) and list(ys) == list(range(0, h - 7, 4)) and q.shape == (len(ys), len(xs))
    for j, y0 in enumerate(ys):
        for i, x0 in enumerate(xs):
            assert abs(q[j, i] / 1048576.0 - _float_ssim(T, F, x0, y0)) <= 2.0 ** -20 + 1e-9, (kind, x0, y0)
    if kind == "identical":
        assert (q == 1 << 20).all()
    if kind == "checker":
        assert (q < 0).all()


def test_the_error_sums_are_a_direct_mse_and_psnr():
    rng = np.random.default_rng(6)
    w, h = 41, 23
    test, ref = qc.images_of("random", w, h, rng)
    classes = qc.classes_of("all_five", w, h, rng)
    s = qr.quality(test, ref, classes, (20, 11), dict(flags=qr.PROFILE, ring_width=3))
    rgb = lambda a: a.view(np.uint8).reshape(h, w, 4)[..., :3].astype(np.float64)
    d2 = (rgb(test) - rgb(ref)) ** 2
    for k in list(range(5)) + [-1]:
        m = (classes == k) if k >= 0 else (classes != qr.UNWRITTEN)
        want = d2[m].mean()
        assert math.isclose(qr.mse(s, k), want, rel_tol=1e-12)
        assert math.isclose(qr.psnr(s, k), 10 * math.log10(255.0 ** 2 / want), rel_tol=1e-12)
    assert sum(s["pixels"]) == w * h == sum(s["ring_pixels"]) and sum(s["ring_sq_err"]) == int(d2.sum()) == sum(sum(c) for c in s["sq_err"])
    assert s["windows"] == [0] * 5 and s["ssim_q20"] == [0] * 5
    # the profile: rings of a direct float distance, away from the ring borders
    yy, xx = np.mgrid[0:h, 0:w]
    dist = np.hypot(xx - 20.0, yy - 11.0)
    ring = qr.ring_map(w, h, (20, 11), 3)
    inner = np.abs(dist / 3 - np.round(dist / 3)) > 1e-6
    assert np.array_equal(ring[inner], np.minimum(63, np.floor(dist / 3))[inner].astype(np.int64))


def test_the_ring_of_a_pixel_in_python_integers():
    """ring_map (64-bit arrays, with the far shortcut) is ring_of (Python integers, math.isqrt) for gazes in the frame, off it on
    both sides, at the int32 limits, and at distances around the shortcut's 2^22."""
    w, h = 9, 7
    u32 = lambda v: v & 0xffffffff
    gazes = [(4, 3), (0, 0), (u32(-1), u32(-1)), (u32(-(1 << 22)), 2), (u32(-(1 << 22) + 3), 2), ((1 << 22) + 5, u32(-(1 << 22) - 1)),
             (0x7fffffff, 0x80000000), (0x80000000, 0x7fffffff), (3, (1 << 22) - 2), (63 * 65536 + 3, 1), (63 * 65536 - 3, 0)]
    for gaze in gazes:
        for rw in (1, 2, 16, 4097, 65535, 65536):
            got = qr.ring_map(w, h, gaze, rw)
            want = np.array([[qr.ring_of(x, y, gaze, rw) for x in range(w)] for y in range(h)])
            assert np.array_equal(got, want), (gaze, rw)
    d = np.array([0, 1, 2, 3, 4, 8, 9, 15, 16, (1 << 52) - 1, (1 << 45) + 7, (3037000499 ** 2) % (1 << 53), 94906265 ** 2, 94906265 ** 2 - 1], np.int64)
    assert [int(v) for v in qr.isqrt(d)] == [math.isqrt(int(v)) for v in d]


# ---- 2. the host implementation against the restatement -----------------------------------------------------------------------------
def test_the_cases_cover_what_they_claim(cases):
    seen = {(c["cfg"]["flags"], c["cfg"]["ring_width"]) for c in cases}
    assert seen == {(f, r) for f in qc.FLAGS for r in qc.RING_WIDTHS}
    assert {(c["w"], c["h"]) for c in cases} == set(qc.SIZES) and {c["image"] for c in cases} == set(qc.IMAGES)
    assert any(qr.as_int32(c["gaze"][0]) < 0 for c in cases) and any(c["gaze"] == (0, 0) for c in cases)
    assert any(c["gaze"][0] >= c["w"] and qr.as_int32(c["gaze"][0]) > 0 for c in cases)
    for c in cases:
        present = set(np.unique(c["classes"]).tolist())
        if c["w"] * c["h"] >= 5:
            assert present == ({0, 1, 2, 3, 4} if c["class_map"] == "all_five" else {0, 1, 2, 4}), c["label"]


def test_host_equals_the_restatement_bit_for_bit(cases, loader):
    for c in cases:
        want = qr.quality(c["test"], c["ref"], c["classes"], c["gaze"], c["cfg"])
        rc, got = qc.host_quality(loader, c["test"], c["ref"], c["classes"], c["gaze"], c["cfg"])
        assert rc == 0, c["label"]
        assert got.as_dict() == want, c["label"]
        assert bytes(got) == bytes(qc.sums_of_dict(want)), c["label"]
        flags = c["cfg"]["flags"]
        n_windows = (0 if c["w"] < 8 or c["h"] < 8 else ((c["w"] - 8) // 4 + 1) * ((c["h"] - 8) // 4 + 1)) if flags & qr.SSIM else 0
        assert sum(want["windows"]) == n_windows and sum(want["ring_pixels"]) == (c["w"] * c["h"] if flags & qr.PROFILE else 0), c["label"]
        if c["image"] in ("identical", "alpha"):              # no error anywhere; every window's q is exactly 2^20
            assert want["differing"] == [0] * 5 and want["max_err"] == [0] * 5 and want["sq_err"] == [[0, 0, 0]] * 5, c["label"]
            assert want["ring_sq_err"] == [0] * 64 and want["ssim_q20"] == [n << 20 for n in want["windows"]], c["label"]
        if c["image"] == "black_white":
            assert want["max_err"] == [255 if n else 0 for n in want["pixels"]] and want["differing"] == want["pixels"], c["label"]
            assert want["sq_err"] == [[n * 65025] * 3 for n in want["pixels"]], c["label"]
        if c["image"] == "checker" and n_windows:
            assert sum(want["ssim_q20"]) < 0 and all(q <= 0 for q in want["ssim_q20"]), c["label"]


def test_host_without_classes_counts_every_pixel_uniform(cases, loader):
    c = cases[-1]
    rc, got = qc.host_quality(loader, c["test"], c["ref"], None, c["gaze"], c["cfg"])
    want = qr.quality(c["test"], c["ref"], np.full((c["h"], c["w"]), qr.UNIFORM), c["gaze"], c["cfg"])
    assert rc == 0 and got.as_dict() == want and got.pixels[qr.UNIFORM] == c["w"] * c["h"]


def test_host_rejections_leave_the_record_alone(loader):
    rng = np.random.default_rng(8)
    test, ref = qc.images_of("random", 12, 9, rng)
    k = qc.classes_of("all_five", 12, 9, rng)
    s = abi.QualitySums()
    C.memset(C.byref(s), 0x5a, C.sizeof(s))
    before = bytes(s)
    good = qc.config_of(qr.DEFAULTS)

    def call(test_p=test.ctypes.data, ref_p=ref.ctypes.data, w=12, h=9, k_p=k.ctypes.data, cfg=good, out=C.byref(s)):
        return loader.fovpt_quality_host(test_p, ref_p, w, h, k_p, 3, 4, C.byref(cfg) if cfg is not None else None, out)

    bad = []
    for f, v in (("flags", 4), ("flags", -1), ("flags", 1 << 30), ("ring_width", 0), ("ring_width", -5), ("ring_width", 65537)):
        cfg = good.copy()
        setattr(cfg, f, v)
        bad.append(cfg)
    for i in range(6):
        cfg = good.copy()
        cfg._reserved[i] = 1
        bad.append(cfg)
    for cfg in bad:
        assert call(cfg=cfg) == E_INVALID
    assert call(test_p=None) == E_INVALID and call(ref_p=None) == E_INVALID and call(cfg=None) == E_INVALID and call(out=None) == E_INVALID
    assert call(w=0) == E_INVALID and call(h=0) == E_INVALID and call(w=-12) == E_INVALID and call(w=1 << 16, h=1 << 15) == E_INVALID
    k2 = k.copy()
    k2[4, 5] = 5
    assert call(k_p=k2.ctypes.data) == E_INVALID
    assert bytes(s) == before and b"fovpt_quality_host" in loader.fovpt_last_error(None)
    assert call() == 0 and bytes(s) != before


# ---- 3. the scores --------------------------------------------------------------------------------------------------------------------
def _hand_made():
    d = dict(pixels=[100, 50, 0, 10, 7], differing=[3, 0, 0, 10, 7], sq_err=[[300, 0, 600], [0, 0, 0], [0, 0, 0], [65025 * 10] * 3, [7, 7, 7]],
             max_err=[20, 0, 0, 255, 1], _pad=0, windows=[4, 2, 0, 0, 1], ssim_q20=[4 << 20, 1 << 19, 0, 0, -(1 << 20)],
             ring_pixels=[0] * 64, ring_sq_err=[0] * 64, width=16, height=11, ring_width=16, flags=3)
    return d, qc.sums_of_dict(d)


def test_the_scores_of_hand_made_sums(loader):
    d, s = _hand_made()
    same = lambda a, b: (a != a and b != b) or a == b
    for k in range(-1, 5):
        for name in ("mse", "psnr", "ssim"):
            got = getattr(loader, "fovpt_quality_" + name)(C.byref(s), k)
            assert same(got, getattr(qr, name)(d, k)), (name, k, got)
    L = loader
    assert L.fovpt_quality_mse(C.byref(s), 0) == 3.0 and L.fovpt_quality_psnr(C.byref(s), 0) == 10.0 * math.log10(65025.0 / 3.0)
    assert L.fovpt_quality_mse(C.byref(s), 1) == 0.0 and L.fovpt_quality_psnr(C.byref(s), 1) == math.inf            # mse 0
    assert all(math.isnan(getattr(L, "fovpt_quality_" + n)(C.byref(s), 2)) for n in ("mse", "psnr", "ssim"))        # an empty class
    assert L.fovpt_quality_mse(C.byref(s), 3) == 65025.0 and L.fovpt_quality_psnr(C.byref(s), 3) == 0.0
    assert L.fovpt_quality_ssim(C.byref(s), 0) == 1.0 and L.fovpt_quality_ssim(C.byref(s), 1) == 0.25 and L.fovpt_quality_ssim(C.byref(s), 4) == -1.0
    assert math.isnan(L.fovpt_quality_ssim(C.byref(s), 3))                                                           # pixels, but no window
    assert L.fovpt_quality_mse(C.byref(s), -1) == (900 + 3 * 650250) / (3.0 * 160)                                   # all but UNWRITTEN
    assert L.fovpt_quality_ssim(C.byref(s), -1) == ((4 << 20) + (1 << 19)) / (1048576.0 * 6)
    for k in (-2, 5, 1000):
        assert all(math.isnan(getattr(L, "fovpt_quality_" + n)(C.byref(s), k)) for n in ("mse", "psnr", "ssim"))
    assert math.isnan(L.fovpt_quality_mse(None, 0)) and math.isnan(L.fovpt_quality_ssim(None, -1))
    for wts in ([1, 1, 1, 1, 1], [4, 2, 1, 1, 0], [0, 0, 0, 1, 0], [0.5, 0, 0, 0, 0.25]):
        w = (C.c_double * 5)(*wts)
        assert L.fovpt_quality_score(C.byref(s), w) == qr.score(d, wts), wts
    assert L.fovpt_quality_score(C.byref(s), (C.c_double * 5)(1, 0, 0, 0, 0)) == 3.0
    assert math.isnan(L.fovpt_quality_score(C.byref(s), (C.c_double * 5)(0, 0, 1, 0, 0)))                            # weight on an empty class alone
    assert math.isnan(L.fovpt_quality_score(C.byref(s), (C.c_double * 5)())) and math.isnan(L.fovpt_quality_score(C.byref(s), None))


def test_the_renderers_scores_are_the_librarys():
    from fovpathtracing_optixcodelatest_amd import renderer
    d, s = _hand_made()
    got = renderer.SampleRenderer.quality_scores(s)
    assert got["mse"]["fovea"] == 3.0 and got["psnr"]["middle"] == math.inf and math.isnan(got["ssim"]["periphery"]) and got["ssim"]["unwritten"] == -1.0
    assert got["mse"]["all"] == qr.mse(d, -1) and len(got["profile_mse"]) == 64 and all(math.isnan(v) for v in got["profile_mse"])
    assert renderer.SampleRenderer.quality_score(s, [4, 2, 1, 1, 0]) == qr.score(d, [4, 2, 1, 1, 0])


# ---- 4. the host implementation under the sanitizers ------------------------------------------------------------------------------------
def test_host_under_the_sanitizers(cases, tmp_path):
    """csrc/quality_host.cpp in a stand-alone program (tests/cpp/quality_host_test.cpp) built with AddressSanitizer and
    UndefinedBehaviorSanitizer, on every case above: the images in heap blocks of their exact size.  Nothing is preloaded and
    nothing is loaded into Python."""
    exe, data = str(tmp_path / "quality_host_test"), str(tmp_path / "cases.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-ffp-contract=off", os.path.join(CSRC, "quality_host.cpp"), os.path.join(ROOT, "tests", "cpp", "quality_host_test.cpp"), "-o", exe])
    qc.write_cases(data, cases)
    res = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    assert "runtime error" not in res.stderr and "Sanitizer" not in res.stderr, res.stderr[-3000:]
    f = dict(kv.split("=") for kv in res.stdout.split())
    assert int(f["cases"]) == len(cases) and int(f["bad"]) == 0 and int(f["refused"]) == 11 * len(cases) and f["error"] == "set", res.stdout


# ---- 5. the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_struct_mirrors_match_the_header():
    structs = [("fovpt_quality_config", abi.QualityConfig), ("fovpt_quality_sums", abi.QualitySums)]
    for (cname, cls), got in zip(structs, header_layout.layouts(*structs)):
        assert got[0] == C.sizeof(cls) and got[1:] == [getattr(cls, n).offset for n, _ in cls._fields_], cname
    assert C.sizeof(abi.QualityConfig) == 32 and C.sizeof(abi.QualitySums) == 1344
    hdr = open(os.path.join(ROOT, "include", "fovpt.h")).read()
    assert re.search(r"static_assert\(sizeof\(fovpt_quality_config\) == 32", hdr) and re.search(r"static_assert\(sizeof\(fovpt_quality_sums\) == 1344", hdr)
    for name, value in (("QUALITY_SSIM", 1), ("QUALITY_PROFILE", 2), ("QUALITY_CLASSES", 5), ("QUALITY_FOVEA", 0), ("QUALITY_MIDDLE", 1), ("QUALITY_PERIPHERY", 2),
                        ("QUALITY_UNIFORM", 3), ("QUALITY_UNWRITTEN", 4), ("QUALITY_RINGS", 64), ("QUALITY_MAX_RING_WIDTH", 65536)):
        assert re.search(r"#define FOVPT_%s\s+%d\b" % (name, value), hdr), name
        assert getattr(abi, name) == value
    assert (qr.SSIM, qr.PROFILE, qr.CLASSES, qr.RINGS, qr.MAX_RING_WIDTH) == (abi.QUALITY_SSIM, abi.QUALITY_PROFILE, 5, 64, 65536)
    names = subprocess.check_output(["nm", "-D", "--defined-only", lib.SO_PATH], text=True)
    for sym in ("fovpt_quality_defaults", "fovpt_quality", "fovpt_quality_read", "fovpt_quality_host", "fovpt_quality_mse", "fovpt_quality_psnr",
                "fovpt_quality_ssim", "fovpt_quality_score"):
        assert re.search(r"\bT %s\b" % sym, names), sym
        assert sym in lib.EXPORTS
    loader_names = subprocess.check_output(["nm", "-D", "--defined-only", lib.LOADER_SO_PATH], text=True)
    for sym in lib.QUALITY_HOST_EXPORTS:
        assert re.search(r"\bT %s\b" % sym, loader_names), sym
    assert "k_quality_tile" in subprocess.check_output(["strings", lib.SO_PATH], text=True)


def test_the_defaults():
    from fovpathtracing_optixcodelatest_amd import renderer
    d = renderer.SampleRenderer.quality_defaults()
    assert (d.flags, d.ring_width, list(d._reserved)) == (abi.QUALITY_SSIM | abi.QUALITY_PROFILE, 16, [0] * 6)
    assert (d.flags, d.ring_width) == (qr.DEFAULTS["flags"], qr.DEFAULTS["ring_width"])
    assert lib.load().fovpt_quality_defaults(None) == E_INVALID
    hdr = open(os.path.join(ROOT, "include", "fovpt.h")).read()
    for word in ("isqrt(d2) / ring_width", "(54 R + 183 G + 19 B + 128) >> 8", "C1 = 26634, C2 = 239708", "2 (64 sxy - sx sy) + C2", "* 1048576.0)"):
        assert word in hdr, word                              # the header's statement of the definition names what the restatement's does


def test_the_dropin_header_compiles():
    src = '#include "SimplePathtracer.h"\nvoid f(SampleRenderer& s, const uint32_t* ref, const uint32_t* test, fovpt_quality_sums* dev, uint8_t* cls) { ' \
          'fovpt_quality_config qc = SampleRenderer::qualityDefaults(); qc.ring_width = 8; fovpt_quality_sums out = s.measureQuality(ref); ' \
          'out = s.measureQuality(ref, test, &qc, cls); s.qualityAsync(ref, test, &qc, dev, cls); out = s.readQuality(); ' \
          'double m = fovpt_quality_mse(&out, -1); (void)m; }\n'
    header_layout.syntax_check(src)
