"""fovpt_lens without a GPU: the restatement (tests/lens_ref.py) on hand-computed cases -- the identity, the shared lookup of equal
chroma factors, the homography of a camera onto itself, one texel moved by a barrel and by a pincushion polynomial, the Catmull-Rom
weights, the all-border windows --, the defaults through ctypes, the struct mirror against the header, the prototypes, the frame
fitting helper, the rejections that need no device, the C++ drop-in, and the index function of the kernel swept by a stand-alone
host program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import header_layout
import lens_ref as lr
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fovpathtracing_optixcodelatest_amd", "csrc")
f32 = np.float32
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
SIZES = [(1, 1), (2, 1), (1, 3), (33, 17), (193, 109)]
IDENTITY = dict(k=(1.0, 0.0, 0.0, 0.0), chroma=(1.0, 1.0, 1.0))
CAMERA = dict(eye=(4.0, 3.0, 6.0), U=(0.55, 0.0, -0.37), V=(-0.1, 0.35, -0.15), W=(-4.0, -2.5, -6.0))


@pytest.fixture(scope="module")
def so():
    lib.build()
    return lib.load()


def image(w, h, seed=0):
    c = np.random.default_rng(seed).uniform(0.05, 4.0, (h, w, 4)).astype(np.float32)
    c[..., 3] = 1.0
    return c


# ---- the definition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_nearest_with_the_identity_polynomial_returns_the_input(size):
    w, h = size
    color = image(w, h)
    o = lr.lens(None, color, lr.config(filter=lr.NEAREST, **IDENTITY))
    assert np.array_equal(bits(o["color"]), bits(color))
    assert o["valid"].all() and o["inside"].all() and (o["border_taps"] == 0).all()
    ys, xs = np.mgrid[0:h, 0:w]
    assert np.array_equal(o["x0"][..., 1], xs) and np.array_equal(o["y0"][..., 2], ys)


@pytest.mark.parametrize("flt", [lr.NEAREST, lr.BILINEAR, lr.BICUBIC])
def test_equal_chroma_factors_share_one_lookup(flt):
    color = image(33, 17, 1)
    for chroma in ((1.0, 1.0, 1.0), (1.014, 1.014, 1.014)):
        d = lr.config(filter=flt, chroma=chroma, scale=(1.0, 17 / 33.0), src_scale=(0.7, 0.7 * 33 / 17.0))
        shared, each = lr.lens(None, color, d, share=True), lr.lens(None, color, d, share=False)
        assert np.array_equal(bits(shared["color"]), bits(each["color"]))
        assert np.array_equal(shared["valid"], each["valid"]) and np.array_equal(bits(shared["fx"]), bits(each["fx"]))
        assert shared["valid"].any() and (shared["border_taps"] > 0).any() if flt != lr.NEAREST else shared["valid"].any()
    assert not lr.same_bits((0.0, -0.0, 0.0)) and lr.same_bits((1.0, 1.0, 1.0))    # equal BITS: 0 and -0 are two factors


def test_a_camera_onto_itself_is_the_identity_homography():
    H = lr.homography(CAMERA, CAMERA)
    M = lr.tr.camera_inverse(CAMERA["U"], CAMERA["V"], CAMERA["W"]).astype(np.float64)
    B = np.array([CAMERA[n] for n in ("U", "V", "W")], np.float32).astype(np.float64).T
    bound = (np.abs(M) @ np.abs(B)) * 2.0 ** -23 + 2.0 ** -24            # every entry of M is off by half an ulp at most; H's own rounding
    assert (np.abs(H.astype(np.float64) - np.eye(3)) <= bound).all() and bound.max() < 1e-5
    color = image(33, 17, 2)
    d = lr.config(filter=lr.NEAREST, **IDENTITY)
    with_to, without = lr.lens(None, color, d, CAMERA, CAMERA), lr.lens(None, color, d)
    assert np.array_equal(bits(with_to["color"]), bits(without["color"])) and with_to["valid"].all()
    assert np.array_equal(bits(without["color"]), bits(color))
    assert lr.homography(dict(U=(1, 0, 0), V=(2, 0, 0), W=(0, 0, 1)), CAMERA) is None      # a singular rendered camera


def test_a_barrel_and_a_pincushion_move_a_texel_to_the_hand_computed_pixel():
    # 16 x 16, destination pixel (12, 8): nx = 25/16 - 1 = 0.5625, ny = 17/16 - 1 = 0.0625, r2 = 0.3203125, every step exact.
    # k1 = 1: f = 1.3203125, sx = 0.74267578125, sy = 0.08251953125, fx = 13.44140625, fy = 8.16015625: the texel (13, 8)
    # k1 = -0.5: f = 0.83984375, sx = 0.472412109375, sy = 0.052490234375, fx = 11.279296875, fy = 7.919921875: the texel (11, 8)
    for k1, src, fx, fy in ((1.0, (13, 8), 13.44140625, 8.16015625), (-0.5, (11, 8), 11.279296875, 7.919921875)):
        color = np.zeros((16, 16, 4), np.float32)
        color[src[1], src[0], :3] = (1.0, 2.0, 4.0)
        o = lr.lens(None, color, lr.config(filter=lr.NEAREST, k=(1.0, k1, 0.0, 0.0), chroma=(1.0, 1.0, 1.0)))
        assert (o["fx"][8, 12] == f32(fx)).all() and (o["fy"][8, 12] == f32(fy)).all()
        assert o["color"][8, 12].tolist() == [1.0, 2.0, 4.0, 1.0]
        assert (o["x0"][8, 12] == src[0]).all() and (o["y0"][8, 12] == src[1]).all()
        o = lr.lens(None, color, lr.config(filter=lr.BILINEAR, k=(1.0, k1, 0.0, 0.0), chroma=(1.0, 1.0, 1.0)))
        tx, ty = f32(fx) - np.floor(f32(fx)), f32(fy) - np.floor(f32(fy))
        wx = tx if src[0] > np.floor(fx) else f32(1) - tx                  # the weight of the texel among the window's four
        wy = ty if src[1] > np.floor(fy) else f32(1) - ty
        assert o["color"][8, 12, 0] == f32(wy * wx) or abs(o["color"][8, 12, 0] - float(wx) * float(wy)) < 1e-6
    # distinct chroma factors: the channels read different texels
    color = image(16, 16, 3)
    o = lr.lens(None, color, lr.config(filter=lr.NEAREST, k=(1.0, 1.0, 0.0, 0.0), chroma=(0.9, 1.0, 1.1)))
    assert ((o["x0"][..., 0] != o["x0"][..., 2]) & o["valid"][..., 0] & o["valid"][..., 2]).any()
    assert o["color"][8, 12, 1] == color[8, 13, 1]


def test_the_catmull_rom_weights_sum_to_one_and_reproduce_a_constant():
    t = np.concatenate([np.linspace(0, 1, 100001).astype(np.float32), np.float32([0.0, 1.0, 0.5, np.nextafter(f32(1), f32(0)), 2.0 ** -24])])
    w = lr.cubic_weights(t)
    total = ((w[0] + w[1]) + w[2]) + w[3]
    assert total.dtype == np.float32 and np.abs(total.astype(np.float64) - 1.0).max() <= 2 * 2.0 ** -23
    w0 = lr.cubic_weights(f32(0.0))
    assert [float(x) for x in w0] == [0.0, 1.0, 0.0, 0.0]
    exact = lambda t: (((-0.5 * t + 1.0) * t - 0.5) * t, ((1.5 * t - 2.5) * t) * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t, ((0.5 * t - 0.5) * t) * t)
    for a, b in zip(w, exact(t.astype(np.float64))):
        assert np.abs(a - b).max() < 1e-6
    # a constant image under a shifted, scaled lookup: fractional t everywhere, and the border equal to the constant.  Two passes,
    # each a sum of four products whose weights are off 1 by 2 ulp at most and round seven times: 16 ulp of the constant bounds it
    const = f32(1.75)
    color = np.full((17, 33, 4), const, np.float32)
    d = lr.config(filter=lr.BICUBIC, **IDENTITY, src_scale=(0.83, 0.71), src_center=(0.013, -0.021), border=(1.75, 1.75, 1.75, 1.0))
    o = lr.lens(None, color, d)
    tx = o["fx"] - np.floor(o["fx"])
    assert ((tx > 0.01) & (tx < 0.99)).mean() > 0.9 and o["valid"].all()
    assert np.abs(o["color"][..., :3].astype(np.float64) - float(const)).max() <= 16 * 2.0 ** -23 * float(const)


@pytest.mark.parametrize("flt", [lr.NEAREST, lr.BILINEAR, lr.BICUBIC])
def test_every_all_border_window_returns_the_border_exactly(flt):
    border = (0.3, 0.7, 1.1, 0.25)
    color = image(33, 17, 4)
    n = lr.TAPS[flt]
    # shifted by about a frame: part of the positions leaves the accepted range, part stays inside it with a window beside the frame
    for centre in ((1.9, 0.0), (-1.95, 0.0), (0.0, 1.93), (0.0, -1.9), (1.0, 1.0)):
        d = lr.config(filter=flt, **IDENTITY, src_center=centre, border=border)
        o = lr.lens(None, color, d)
        empty = o["valid"] & (o["border_taps"] == n * n)
        assert (~o["valid"]).any() or empty.any()
        for c in range(3):
            assert (bits(o["color"][..., c][empty[..., c]]) == bits([border[c]])[0]).all()
            assert (bits(o["color"][..., c][~o["valid"][..., c]]) == bits([border[c]])[0]).all()
        if flt == lr.BILINEAR and centre[0] != 0.0 and centre[1] == 0.0:
            assert empty.any(), centre                                     # valid positions whose whole window lies beside the frame
        assert (o["color"][..., 3] == 1.0).all()
    # 32 x 16 shifted by exactly two pixels: the last column's fx is w + 1, the one position whose Catmull-Rom window (w .. w + 3)
    # misses the frame; the rows of those windows are combined with fractional y weights, which round: the rule is what keeps them exact
    o = lr.lens(None, image(32, 16, 5), lr.config(filter=flt, **IDENTITY, src_center=(0.125, 0.01), border=border))
    assert (o["fx"][:, 31] == 33.0).all() and o["valid"][:, 31].all() and (o["border_taps"][:, 31] == n * n).all()
    assert (bits(o["color"][:, 31, :3]) == bits(border[:3])).all()
    # outside the lens: all four components of the border
    o = lr.lens(None, color, lr.config(filter=flt, clip_r2=0.5, scale=(1.0, 17 / 33.0), border=border))
    assert o["inside"].any() and (~o["inside"]).any()
    assert (bits(o["color"][~o["inside"]]) == bits(border)).all() and (o["color"][o["inside"]][:, 3] == 1.0).all()
    # coefficients that are valid but overflow: every channel invalid (the axis off every pixel centre: at r2 = 0 nothing overflows)
    o = lr.lens(None, color, lr.config(filter=flt, k=(1.0, 0.0, 0.0, 3e38), scale=(1000.0, 1000.0), center=(0.003, 0.003), border=border))
    assert not o["valid"].any() and (bits(o["color"][..., :3]) == bits(border[:3])).all()


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_lens_defaults_are_the_documented_ones(so):
    d = abi.LensConfig()
    C.memset(C.byref(d), 0xff, C.sizeof(d))
    assert so.fovpt_lens_defaults(C.byref(d)) == 0
    assert C.sizeof(d) == C.sizeof(abi.LensConfig) == 128
    got = d.as_dict()
    assert set(got) == set(lr.DEFAULTS)
    for k, v in lr.DEFAULTS.items():
        want = tuple(float(f32(x)) for x in v) if isinstance(v, tuple) else v
        assert got[k] == want, k
    assert (d.filter, d.encode) == (abi.LENS_BILINEAR, abi.LENS_ENCODE_DISPLAY) == (1, 0)
    assert tuple(d.k) == tuple(float(f32(x)) for x in (1.0, 0.22, 0.24, 0.0)) and tuple(d.chroma) == tuple(float(f32(x)) for x in (0.996, 1.0, 1.014))
    assert d.clip_r2 == float("inf") and tuple(d.border) == (0.0, 0.0, 0.0, 1.0)
    assert list(d._reserved0) == [0, 0] and list(d._reserved) == [0] * 8
    assert so.fovpt_lens_defaults(None) == -1
    assert (abi.LENS_NEAREST, abi.LENS_BILINEAR, abi.LENS_BICUBIC, abi.LENS_ENCODE_DISPLAY, abi.LENS_ENCODE_RESOLVE) == \
           (lr.NEAREST, lr.BILINEAR, lr.BICUBIC, lr.ENCODE_DISPLAY, lr.ENCODE_RESOLVE) == (0, 1, 2, 0, 1)


def test_lens_for_frame_maps_the_edge_mid_points_to_themselves(so):
    d = renderer.SampleRenderer.lens_defaults()
    c = renderer.SampleRenderer.lens_for_frame(d, 1920, 1080)
    f1 = 1.0 + 0.22 + 0.24
    assert c.scale[0] == 1.0 and c.scale[1] == f32(1080 / 1920.0)
    assert abs(c.src_scale[0] * f1 - 1.0) < 1e-6 and abs(c.src_scale[1] * f1 - 1920 / 1080.0) < 1e-6
    assert d.scale[1] == 1.0 and d.src_scale[0] == 1.0                     # a copy: the argument is as it was
    # the mid-point of the right edge: px = 1, py = 0, r2 = 1, green's factor is 1
    assert abs(float(lr.poly(tuple(c.k), f32(1.0))) * c.src_scale[0] - 1.0) < 1e-6
    # a round lens: a step of one pixel is the same lens radius along both axes
    w, h = 1920, 1080
    assert abs((2.0 / w) * c.scale[0] - (2.0 / h) * c.scale[1]) < 1e-9


def test_lens_rejects_what_needs_no_device(so):
    d, lp = abi.LensConfig(), abi.LaunchParams()
    so.fovpt_lens_defaults(C.byref(d))
    assert so.fovpt_lens(None, C.byref(lp), C.byref(d), None, None, None, None) == -1
    col, rgba = C.c_void_p(), C.c_void_p()
    assert so.fovpt_lens_buffers(None, C.byref(col), C.byref(rgba)) == -1


def _args(hdr, name):
    m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
    assert m, "fovpt.h does not declare %s" % name
    return [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", a).strip()) for a in m.group(1).replace("\n", " ").split(",")]


def test_the_prototypes_agree_everywhere(so):
    hdr = open(os.path.join(ROOT, "include", "fovpt.h")).read()
    assert _args(hdr, "fovpt_lens_defaults") == ["fovpt_lens_config* out"]
    assert _args(hdr, "fovpt_lens") == ["fovpt_ctx* ctx", "const fovpt_launch_params* lp", "const fovpt_lens_config* lc", "const fovpt_warp_camera* to",
                                        "const fovpt_float4* in_color", "fovpt_float4* out_color", "uint32_t* out_rgba"]
    assert _args(hdr, "fovpt_lens_buffers") == ["fovpt_ctx* ctx", "fovpt_float4** color", "uint32_t** rgba"]
    for name, value in (("LENS_NEAREST", 0), ("LENS_BILINEAR", 1), ("LENS_BICUBIC", 2), ("LENS_ENCODE_DISPLAY", 0), ("LENS_ENCODE_RESOLVE", 1)):
        assert re.search(r"#define FOVPT_%s\s+%d\b" % (name, value), hdr)
        assert getattr(abi, name) == value
    vp = C.c_void_p
    assert list(so.fovpt_lens.argtypes) == [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.LensConfig), C.POINTER(abi.WarpCamera), vp, vp, vp]
    names = subprocess.check_output(["nm", "-D", "--defined-only", lib.SO_PATH], text=True)
    for sym in ("fovpt_lens_defaults", "fovpt_lens", "fovpt_lens_buffers"):
        assert re.search(r"\bT %s\b" % sym, names), sym
        assert getattr(so, sym).restype == C.c_int and sym in lib.EXPORTS
    assert "k_lens" in subprocess.check_output(["strings", lib.SO_PATH], text=True)
    # the header's statement of the definition names what the restatement's does
    for word in ("clip_r2", "src_scale", "chroma[c]", "(w0 * a0 + w1 * a1) + w2 * a2) + w3 * a3", "fx <= (float)w + 1.0f"):
        assert word in hdr, word


def test_the_struct_mirror_matches_the_header():
    names = [f[0] for f in abi.LensConfig._fields_]
    got = header_layout.layout("fovpt_lens_config", abi.LensConfig)
    assert got[0] == C.sizeof(abi.LensConfig) == 128
    assert got[1:] == [getattr(abi.LensConfig, n).offset for n in names]
    hdr = open(os.path.join(ROOT, "include", "fovpt.h")).read()
    assert re.search(r"static_assert\(sizeof\(fovpt_lens_config\) == 128", hdr)


def test_the_dropin_header_compiles():
    src = '#include "SimplePathtracer.h"\nvoid f(SampleRenderer& s, const sutil::Camera& cam, fovpt_float4* c, uint32_t* h) { s.lens(); s.lens(&cam); ' \
          'fovpt_lens_config lc = SampleRenderer::lensDefaults(); lc.filter = FOVPT_LENS_BICUBIC; lc.encode = FOVPT_LENS_ENCODE_RESOLVE; ' \
          'lc = s.lensForFrame(lc); s.lens(lc); s.lens(lc, &cam, c); fovpt_float4* oc; uint32_t* op; s.lensBuffers(&oc, &op); s.downloadLens(c, h); }\n'
    header_layout.syntax_check(src)


# ---- the kernel's index function on the host -------------------------------------------------------------------------------------------
def test_the_index_function_under_the_host_sanitizers(tmp_path):
    """tests/cpp/lens_taps_test.cpp: csrc/fovpt_lens_taps.h, the function k_lens takes its taps from, swept over the floats around
    the frame's edges and the values no conversion to an integer survives; a stand-alone program, nothing preloaded."""
    exe = str(tmp_path / "lens_taps_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "lens_taps_test.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(res.stdout[-500:], res.stderr[-2000:])
    assert res.returncode == 0 and res.stdout.startswith("ok: "), res.stdout + res.stderr
