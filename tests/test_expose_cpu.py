"""fovpt_expose without a GPU: the restatement (tests/expose_ref.py) on hand-computed cases, the defaults through ctypes, the
struct mirrors against the header, the prototypes and the C++ drop-in."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import header_layout
import expose_ref as ex
from fovpathtracing_optixcodelatest_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def so():
    lib.build()
    return lib.load()


def cfg(**kw):
    return dict(ex.DEFAULTS, **kw)


# ---- the restatement on hand-computed cases ---------------------------------------------------------------------------------------
def test_bin_edges():
    denormal = np.uint32(1).view(np.float32)
    L = np.array([1.0, 1.5, 2.0 ** -17, denormal, 65536.0, np.inf, 2.0 ** -16, 65535.0, 2.0, 0.5, np.nextafter(f32(1.5), f32(0))], np.float32)
    counts, b = ex.bins(L)
    assert counts.all()
    assert b.tolist() == [128, 132, 0, 0, 255, 255, 0, 255, 136, 120, 131]
    counts, _ = ex.bins(np.array([np.nan, 0.0, -0.0, -1.0, -np.inf], np.float32))
    assert not counts.any()


def test_luminance_is_left_to_right_in_float32():
    c = np.array([[0.3, 0.7, 0.9, 5.0]], np.float32)
    want = f32(f32(f32(0.2126) * c[0, 0]) + f32(f32(0.7152) * c[0, 1])) + f32(f32(0.0722) * c[0, 2])
    assert ex.luminance(c)[0] == want and ex.luminance(c).dtype == np.float32


def test_a_constant_image_of_one_meters_a_sixteenth(oracle):
    img = np.ones((5, 7, 4), np.float32)
    d = cfg(metering=ex.FRAME)
    h = ex.histogram(img, d)
    assert h[128] == 35 and h.sum() == 35 and h.dtype == np.uint64
    ev, T = ex.trimmed_mean(h, d)
    assert ev == f32(0.0625) and T == 35                      # bin 128's centre: (2 * 128 + 1) / 16 - 16
    out, rgba, h2, st = ex.expose(oracle, img, d, ex.new_state())
    assert st["ev"] == st["ev_metered"] == f32(0.0625) and st["steps"] == 1 and st["weight_total"] == 35
    p = oracle.math_op(ex.OP_POW, np.float32([2.0]), np.float32([0.0625]))[0]
    assert st["exposure"] == f32(0.18) / p and abs(float(st["exposure"]) - 0.18 / 2 ** 0.0625) < 1e-6
    assert (out[..., 3] == 1).all() and np.array_equal(h, h2) and rgba.shape == (5, 7)


def test_permille_cuts_inside_a_bin():
    h = np.zeros(256, np.uint64)
    h[10], h[20] = 10, 10
    # T = 20, a = 5, b = 15: five of bin 10 and five of bin 20; S = 5 * 21 + 5 * 41 = 310, S / 2N = 15.5
    ev, T = ex.trimmed_mean(h, cfg(low_permille=250, high_permille=750, ev_min=-16.0, ev_max=16.0))
    assert T == 20 and ev == f32(-16.0 + 15.5 / 8.0)
    # a = 20 * 333 // 1000 = 6, b = (20 * 501 + 999) // 1000 = 11: four of bin 10, one of bin 20
    ev, _ = ex.trimmed_mean(h, cfg(low_permille=333, high_permille=501, ev_min=-16.0, ev_max=16.0))
    assert ev == f32(np.float64(-16.0) + (np.float64(4 * 21 + 41) / np.float64(10)) / np.float64(8))
    # the clamp
    assert ex.trimmed_mean(h, cfg(ev_min=-3.0, ev_max=2.0))[0] == f32(-3.0)
    # all of the weight in the last bin, the whole range
    h = np.zeros(256, np.uint64)
    h[255] = 3
    assert ex.trimmed_mean(h, cfg(low_permille=0, high_permille=1000, ev_min=-16.0, ev_max=16.0))[0] == f32(-16.0 + 511.0 / 16.0)


def test_gaze_weights():
    fill = np.array([[1, 2, 4, 0]])
    d = cfg(weight_fovea=7, weight_middle=5, weight_periphery=3, weight_uniform=2)
    assert ex.weights(fill, d, 0).tolist() == [[7, 5, 3, 0]]
    assert ex.weights(np.array([[1, 1, 1, 0]]), d, 1).tolist() == [[2, 2, 2, 0]]
    img = np.ones((1, 4, 4), np.float32)
    assert ex.histogram(img, d, fill, 0)[128] == 15 and ex.histogram(img, cfg(metering=ex.FRAME))[128] == 4


def test_nothing_to_meter(oracle):
    black = np.zeros((3, 3, 4), np.float32)
    nan = np.full((3, 3, 4), np.nan, np.float32)
    for img in (black, nan):
        d = cfg(metering=ex.FRAME)
        assert ex.trimmed_mean(ex.histogram(img, d), d) == (None, 0)
        _, _, _, st = ex.expose(oracle, img, d, ex.new_state())
        assert st["ev"] == 0 and st["ev_metered"] == 0 and st["exposure"] == f32(0.18) and st["steps"] == 1
        _, _, _, st = ex.expose(oracle, img, cfg(metering=ex.FRAME, ev_min=2.0, ev_max=3.0), ex.new_state())
        assert st["ev"] == 2                                   # a first step: clamp(0, ev_min, ev_max)
        # a later step keeps its ev, outside the present clamp too
        _, _, _, st = ex.expose(oracle, np.full((3, 3, 4), 4.0, np.float32), d, ex.new_state())
        ev = st["ev"]
        _, _, _, st = ex.expose(oracle, img, cfg(metering=ex.FRAME, ev_min=-1.0, ev_max=1.0), st)
        assert ev == f32(2.0625) and st["ev"] == ev and st["ev_metered"] == ev and st["steps"] == 2 and st["weight_total"] == 0


def test_adaptation_moves_a_share_of_the_way(oracle):
    d = cfg(metering=ex.FRAME, adapt_brighter=0.5, adapt_darker=0.25)
    one, four = np.ones((2, 2, 4), np.float32), np.full((2, 2, 4), 4.0, np.float32)
    _, _, _, st = ex.expose(oracle, one, d, ex.new_state())
    _, _, _, st = ex.expose(oracle, four, d, st)
    assert st["ev_metered"] == f32(2.0625) and st["ev"] == f32(1.0625)                 # brighter: half of the way
    _, _, _, st = ex.expose(oracle, one, d, st)
    assert st["ev"] == f32(0.8125) and st["steps"] == 3                                # darker: a quarter
    out, rgba, h, st2 = ex.expose(oracle, one, cfg(mode=ex.FIXED), st)
    assert st2 is st and h is None


def test_fixed_16_reinhard_white_1_is_the_other_stages_tone_map(oracle):
    rng = np.random.default_rng(5)
    img = rng.uniform(0, 0.3, (9, 11, 4)).astype(np.float32)
    out, rgba, _, _ = ex.expose(oracle, img, cfg(mode=ex.FIXED, exposure=16.0, white=1.0), ex.new_state())
    assert np.array_equal(rgba.reshape(-1), oracle.make_color(img[..., :3].reshape(-1, 3)))
    aces = ex.tone(np.float32([[1.0, 0.0, 0.5, 0.0]]), 1.0, cfg(tone=ex.ACES))
    assert aces[0, 0] == (f32(2.51) + f32(0.03)) / ((f32(2.43) + f32(0.59)) + f32(0.14)) and 0.80 < aces[0, 0] < 0.81 and aces[0, 1] == 0 and aces[0, 3] == 1


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_mirrors_have_the_documented_sizes():
    assert C.sizeof(abi.ExposeConfig) == 80 and C.sizeof(abi.ExposeState) == 32
    assert (abi.ExposeConfig.low_permille.offset, abi.ExposeConfig.key.offset, abi.ExposeState.weight_total.offset) == (32, 48, 16)


def test_expose_defaults_are_the_documented_ones(so):
    d = abi.ExposeConfig()
    C.memset(C.byref(d), 0xff, C.sizeof(d))
    assert so.fovpt_expose_defaults(C.byref(d)) == 0
    assert (d.mode, d.metering, d.tone) == (abi.EXPOSE_AUTO, abi.METER_GAZE, abi.TONE_REINHARD) == (1, 1, 0)
    assert (d.weight_fovea, d.weight_middle, d.weight_periphery, d.weight_uniform) == (64, 8, 1, 1)
    assert (d.low_permille, d.high_permille, d.ev_min, d.ev_max) == (100, 950, -12.0, 12.0)
    assert d.key == f32(0.18) and d.white == f32(1e6) == f32(abi.SIGMA_MAX) and d.exposure == 16.0
    assert d.adapt_brighter == 1.0 and d.adapt_darker == 1.0 and d._reserved0 == 0 and list(d._reserved) == [0, 0, 0]
    got = d.as_dict()
    assert set(got) == set(ex.DEFAULTS)
    for k, v in ex.DEFAULTS.items():
        assert f32(got[k]) == f32(v), k
    assert so.fovpt_expose_defaults(None) == -1
    assert abi.EXPOSE_BINS == ex.BINS == 256


def test_expose_rejects_a_null_context(so):
    d, lp, st = abi.ExposeConfig(), abi.LaunchParams(), abi.ExposeState()
    so.fovpt_expose_defaults(C.byref(d))
    assert so.fovpt_expose(None, C.byref(lp), C.byref(d), None, None, None) == -1
    col, rgba = C.c_void_p(), C.c_void_p()
    assert so.fovpt_expose_buffers(None, C.byref(col), C.byref(rgba)) == -1
    assert so.fovpt_expose_state(None, C.byref(st)) == -1 and so.fovpt_expose_reset(None) == -1


def _args(hdr, name):
    m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
    assert m, "fovpt.h does not declare %s" % name
    return [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", a).strip()) for a in m.group(1).replace("\n", " ").split(",")]


def test_the_prototypes_agree_everywhere(so):
    hdr = open(os.path.join(ROOT, "include", "fovpt.h")).read()
    assert _args(hdr, "fovpt_expose_defaults") == ["fovpt_expose_config* out"]
    assert _args(hdr, "fovpt_expose") == ["fovpt_ctx* ctx", "const fovpt_launch_params* lp", "const fovpt_expose_config* ec",
                                          "const fovpt_float4* in_color", "fovpt_float4* out_color", "uint32_t* out_rgba"]
    assert _args(hdr, "fovpt_expose_buffers") == ["fovpt_ctx* ctx", "fovpt_float4** color", "uint32_t** rgba"]
    assert _args(hdr, "fovpt_expose_state") == ["fovpt_ctx* ctx", "struct fovpt_expose_state* out"]
    assert _args(hdr, "fovpt_expose_reset") == ["fovpt_ctx* ctx"]
    for name, value in (("EXPOSE_FIXED", 0), ("EXPOSE_AUTO", 1), ("METER_FRAME", 0), ("METER_GAZE", 1), ("TONE_REINHARD", 0), ("TONE_ACES", 1),
                        ("EXPOSE_BINS", 256)):
        assert re.search(r"#define FOVPT_%s\s+%d\b" % (name, value), hdr)
        assert getattr(abi, name) == value
    vp = C.c_void_p
    assert list(so.fovpt_expose.argtypes) == [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.ExposeConfig), vp, vp, vp]
    assert list(so.fovpt_expose_state.argtypes) == [vp, C.POINTER(abi.ExposeState)]
    names = subprocess.check_output(["nm", "-D", "--defined-only", lib.SO_PATH], text=True)
    for sym in ("fovpt_expose_defaults", "fovpt_expose", "fovpt_expose_buffers", "fovpt_expose_state", "fovpt_expose_reset"):
        assert re.search(r"\bT %s\b" % sym, names), sym
        assert getattr(so, sym).restype == C.c_int
    kernels = subprocess.check_output(["strings", lib.SO_PATH], text=True)
    for k in ("k_expose_meter", "k_expose_adapt", "k_expose_apply"):
        assert k in kernels, k


def test_the_struct_mirrors_match_the_header():
    for ctype, mirror, size in (("fovpt_expose_config", abi.ExposeConfig, 80), ("struct fovpt_expose_state", abi.ExposeState, 32)):
        names = [f[0] for f in mirror._fields_]
        got = header_layout.layout(ctype, mirror)
        assert got[0] == C.sizeof(mirror) == size
        assert got[1:] == [getattr(mirror, n).offset for n in names]


def test_the_dropin_header_compiles():
    src = '#include "SimplePathtracer.h"\nvoid f(SampleRenderer& s, fovpt_float4* m, uint32_t* h) { s.expose(); fovpt_expose_config ec; ' \
          'fovpt_expose_defaults(&ec); ec.mode = FOVPT_EXPOSE_FIXED; ec.tone = FOVPT_TONE_ACES; ec.metering = FOVPT_METER_FRAME; ' \
          's.expose(ec); s.expose(ec, m); s.exposePost(ec); struct fovpt_expose_state st = s.exposeState(); (void)st.steps; ' \
          's.exposeReset(); s.downloadExposedPixels(h); }\n'
    header_layout.syntax_check(src)
