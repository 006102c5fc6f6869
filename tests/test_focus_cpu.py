"""fovpt_focus without a GPU: the restatement (tests/focus_ref.py) on hand-computed cases -- the meter's bins and ranks, the adapt
step, the radii, the reach of one bright pixel, the foreground / background rule, the summation order and the two shortcuts of
k_focus_gather --, the defaults through ctypes, the struct mirrors against the header, the prototypes, the rejections that need no
device and the C++ drop-in."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import header_layout
import focus_ref as fr
from fovpathtracing_optixcodelatest_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
u32bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def so():
    lib.build()
    return lib.load()


def plane(w, h, t=1.0):
    """A G-buffer whose every pixel is a hit at distance t."""
    pos = np.zeros((h, w, 4), np.float32)
    pos[..., 3] = t
    return dict(prim=np.zeros((h, w), np.uint32), position=pos)


def fixed(**d):
    return fr.config(mode=fr.FIXED, **d)


# ---- the meter ---------------------------------------------------------------------------------------------------------------------
def test_the_bins_are_fovpt_exposes_and_the_centre_has_the_documented_bits():
    # t = 1 has the bits 0x3f800000: (u >> 20) - 888 = 128, the bin [1, 1.125), its centre 1.0625
    gb = plane(9, 9, 1.0)
    h = fr.histogram(gb["prim"], gb["position"][..., 3], (4, 4), 0)
    assert h.sum() == 1 and h[128] == 1
    assert fr.bin_centre(128) == f32(1.0625) and u32bits([fr.bin_centre(128)])[0] == 0x3f880000
    assert fr.bin_centre(0) == f32(2.0 ** -16 * 1.0625) and fr.bin_centre(255) == f32(2.0 ** 15 * 1.9375)
    for t, b in ((1.124, 128), (1.125, 129), (2.0, 136), (0.5, 120), (1e-30, 0), (1e30, 255), (float("inf"), 255)):
        gb = plane(3, 3, t)
        assert fr.histogram(gb["prim"], gb["position"][..., 3], (1, 1), 0)[b] == 1, t
    for t in (0.0, -1.0, float("nan")):                               # t > 0 in float: none of these counts
        gb = plane(3, 3, t)
        assert fr.histogram(gb["prim"], gb["position"][..., 3], (1, 1), 1).sum() == 0, t


def test_the_disc_is_cut_in_integers_and_by_the_frame():
    gb = plane(40, 30, 2.0)
    t = gb["position"][..., 3]
    assert fr.histogram(gb["prim"], t, (20, 15), 2).sum() == 13        # d^2 <= 4: 13 lattice points
    assert fr.histogram(gb["prim"], t, (20, 15), 12).sum() == 441      # d^2 <= 144
    assert fr.histogram(gb["prim"], t, (0, 0), 2).sum() == 6           # the corner keeps a quadrant
    assert fr.histogram(gb["prim"], t, (41, 15), 2).sum() == 1         # outside the frame by two columns: (39, 15) alone
    assert fr.histogram(gb["prim"], t, (43, 15), 2).sum() == 0
    assert fr.histogram(gb["prim"], t, (0xfffffff0, 15), 64).sum() == 0    # the gaze is unsigned: far to the right, not at -16
    gb["prim"][15, 20] = fr.MISS                                       # a miss does not count
    assert fr.histogram(gb["prim"], t, (20, 15), 2).sum() == 12


def test_the_rank_selection():
    h = np.zeros(256, np.int64)
    h[100] = 1
    assert fr.rank_bin(h, 0) == fr.rank_bin(h, 250) == fr.rank_bin(h, 1000) == (100, 1)     # one hit: that bin, whatever the rank
    h[:] = 0
    h[40], h[200] = 30, 70                                             # T = 100: k = rank / 10
    assert fr.rank_bin(h, 0) == (40, 100)
    assert fr.rank_bin(h, 290) == (40, 100)                            # k = 29: the 30th, inside the first bin
    assert fr.rank_bin(h, 299) == (40, 100)
    assert fr.rank_bin(h, 300) == (200, 100)                           # k = 30: the first of the second bin
    assert fr.rank_bin(h, 1000) == (200, 100)                          # k = min(100, 99)
    h[250] = 1
    assert fr.rank_bin(h, 1000) == (250, 101) and fr.rank_bin(h, 999) == (250, 101) and fr.rank_bin(h, 990) == (200, 101)
    assert fr.rank_bin(np.zeros(256, np.int64), 500) == (None, 0)


def test_nothing_to_meter_on_a_first_and_on_a_later_step():
    d = fr.config(focus_default=3.0, adapt_nearer=0.5, adapt_farther=0.25)
    empty = np.zeros(256, np.int64)
    s = fr.adapt(fr.new_state(), empty, d)
    assert (s["focus_metered"], s["inv_focus"], s["focus"], s["count"], s["steps"]) == (f32(3.0), f32(1.0) / f32(3.0), f32(1.0) / (f32(1.0) / f32(3.0)), 0, 1)
    h = np.zeros(256, np.int64)
    h[136] = 5                                                         # t in [2, 2.25): the centre 2.125
    s = fr.adapt(s, h, d)
    later = fr.adapt(s, empty, d)                                      # the step counts, D stays bit for bit
    assert later["steps"] == s["steps"] + 1 and later["count"] == 0
    assert u32bits([later["inv_focus"]])[0] == u32bits([s["inv_focus"]])[0] and later["focus"] == s["focus"]
    assert later["focus_metered"] == s["focus"]


def test_the_adapt_step_with_unequal_rates_in_both_directions():
    d = fr.config(adapt_nearer=0.5, adapt_farther=0.125)
    at = lambda b: np.bincount([b], minlength=256).astype(np.int64)
    s = fr.adapt(fr.new_state(), at(128), d)                           # the first step lands on the metered distance
    assert s["focus_metered"] == f32(1.0625) and s["inv_focus"] == f32(1.0) / f32(1.0625) and s["steps"] == 1
    D0 = s["inv_focus"]
    s = fr.adapt(s, at(120), d)                                        # 0.53125: nearer, D_m > D, half of the way
    Dm = f32(1.0) / f32(0.53125)
    assert Dm > D0 and s["inv_focus"] == f32(D0 + f32(f32(0.5) * f32(Dm - D0))) and s["focus"] == f32(1.0) / s["inv_focus"]
    D1 = s["inv_focus"]
    s = fr.adapt(s, at(144), d)                                        # 4.25: farther, D_m < D, an eighth of the way
    Dm = f32(1.0) / f32(4.25)
    assert Dm < D1 and s["inv_focus"] == f32(D1 + f32(f32(0.125) * f32(Dm - D1))) and s["steps"] == 3
    assert s["focus_metered"] == f32(4.25) and s["count"] == 1


# ---- the radii ---------------------------------------------------------------------------------------------------------------------
def test_a_radius_at_the_cap_below_it_and_on_a_miss():
    prim = np.array([[0, 0, fr.MISS, 0]], np.uint32)
    t = np.array([[1.0, 0.25, -1.0, 2.0]], np.float32)                 # D = 0.5: |1 - .5| = .5, |4 - .5| = 3.5, a miss: |0 - .5|, |.5 - .5| = 0
    r, tp = fr.radius(prim, t, f32(0.5), fr.config(strength=2.0, max_radius=3))
    assert r.tolist() == [[1.0, 3.0, 1.0, 0.0]]
    assert tp[0, 2] == np.inf and tp[0, [0, 1, 3]].tolist() == [1.0, 0.25, 2.0]
    r, _ = fr.radius(prim, t, f32(0.5), fr.config(strength=2.0, max_radius=0))
    assert (r == 0).all()
    r, _ = fr.radius(prim, np.array([[np.nan, 0.0, 1.0, 1.0]], np.float32), f32(0.5), fr.config(strength=2.0, max_radius=3))
    assert r.tolist() == [[3.0, 3.0, 1.0, 1.0]]                        # not s < cap: the cap (the kernel faults on no value of t)


# ---- the gather --------------------------------------------------------------------------------------------------------------------
def test_one_bright_pixel_on_a_plane_with_radius_2():
    w, h = 15, 13
    gb = plane(w, h, 1.0)
    color = np.zeros((h, w, 4), np.float32)
    color[..., 3] = 7.0
    color[6, 7, :3] = (1.0, 2.0, 4.0)
    o = fr.focus(None, gb, (0, 0), color, fixed(focus_distance=0.5, strength=2.0, max_radius=4), fr.new_state())     # r = 2 * |1 - 2| everywhere
    assert (o["coc"] == 2).all()
    ys, xs = np.mgrid[0:h, 0:w]
    reach = (xs - 7) ** 2 + (ys - 6) ** 2 <= 6.25
    assert reach.sum() == 21 and np.array_equal(o["color"][..., 0] > 0, reach)
    assert o["covering"][6, 7] == 21 and (o["covering"][0, :] < 21).all() and o["cut"][0, 0] and not o["cut"][6, 7]
    g = f32(1.0) / f32(6.25)
    den = f32(0)
    for _ in range(21):
        den = f32(den + g)
    for c, v in enumerate((1.0, 2.0, 4.0)):                            # every one of the 21 pixels holds the bright one with weight 1 / 6.25
        assert (u32bits(o["color"][reach][:, c]) == u32bits([f32(g * f32(v)) / den])[0]).all()
    assert (o["color"][..., 3] == 7).all() and not o["acted"].any()


def scene_with_a_rectangle(t_fg, t_bg, w=40, h=30):
    gb = plane(w, h, t_bg)
    fg = np.zeros((h, w), bool)
    fg[10:20, 14:27] = True
    gb["position"][fg, 3] = t_fg
    gb["prim"][fg] = 1
    rng = np.random.default_rng(5)
    color = rng.uniform(0.1, 4, (h, w, 4)).astype(np.float32)
    color[..., 0] = np.where(fg, color[..., 0], 0)                     # red is the foreground's alone
    return gb, fg, color


def test_a_sharp_foreground_keeps_its_pixels_over_a_background_at_the_cap():
    gb, fg, color = scene_with_a_rectangle(1.0, 10.0)
    o = fr.focus(None, gb, (0, 0), color, fixed(focus_distance=1.0, strength=100.0, max_radius=8), fr.new_state())
    assert (o["coc"][fg] == 0).all() and (o["coc"][~fg] == 8).all()
    assert np.array_equal(u32bits(o["color"][fg]), u32bits(color[fg])) and (o["covering"][fg] == 1).all()
    assert (o["color"][~fg][:, 0] == 0).all()                          # no background pixel takes the foreground's red
    assert o["acted"][fg].all() and (o["covering"][~fg] > 100).any()   # the background rule is what keeps the rectangle sharp
    assert not np.array_equal(u32bits(o["color"][~fg]), u32bits(color[~fg]))


def test_a_blurred_foreground_spreads_over_a_sharp_background_by_its_own_radius():
    gb, fg, color = scene_with_a_rectangle(1.0, 4.0)
    o = fr.focus(None, gb, (0, 0), color, fixed(focus_distance=4.0, strength=4.0, max_radius=8), fr.new_state())
    assert (o["coc"][fg] == 3).all() and (o["coc"][~fg] == 0).all()
    red = o["color"][..., 0] > 0
    assert red[15, 11:14].all() and not red[15, 10] and red[15, 27:30].all() and not red[15, 30]      # 3 pixels beside it: d^2 <= 12.25
    assert red[7:10, 20].all() and not red[6, 20] and red[7, 14] and not red[7, 11]                  # (3, 3) from the corner: 18 > 12.25
    far = ~fg & ~red
    assert np.array_equal(u32bits(o["color"][far]), u32bits(color[far]))       # the background beyond stays sharp


def test_strength_0_and_radius_0_return_the_input(so):
    gb, _, color = scene_with_a_rectangle(1.0, 4.0)
    color[3, 3] = (np.inf, 1e-42, 0.0, -2.0)
    for d in (fixed(strength=0.0), fixed(max_radius=0, strength=50.0), fixed(focus_distance=1.0, strength=0.0, max_radius=8)):
        o = fr.focus(None, gb, (0, 0), color, d, fr.new_state())
        assert np.array_equal(u32bits(o["color"]), u32bits(color)) and (o["covering"] == 1).all()
    gb = plane(20, 10, 2.0)                                            # a scene entirely at the focus distance
    o = fr.focus(None, gb, (0, 0), color[:10, :20], fixed(focus_distance=2.0, strength=1e6, max_radius=8), fr.new_state())
    assert np.array_equal(u32bits(o["color"]), u32bits(color[:10, :20]))


def scalar_pixel(color, r, tp, R, x, y, reverse=False):
    """The definition for one pixel as an explicit loop -> its rgb."""
    h, w = r.shape
    taps = [(dx, dy) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]
    den, num, n = f32(0), [f32(0)] * 3, 0
    for dx, dy in (reversed(taps) if reverse else taps):
        qx, qy = x + dx, y + dy
        if not (0 <= qx < w and 0 <= qy < h):
            continue
        rq = r[qy, qx]
        re = (rq if rq < r[y, x] else r[y, x]) if tp[qy, qx] > tp[y, x] else rq
        e = f32(re + f32(0.5))
        e2 = f32(e * e)
        if f32(dx * dx + dy * dy) <= e2:
            g = f32(f32(1.0) / e2)
            den = f32(den + g)
            num = [f32(num[c] + f32(g * color[qy, qx, c])) for c in range(3)]
            n += 1
    return [color[y, x, c] if n == 1 else f32(num[c] / den) for c in range(3)]


def random_scene(w, h, seed, strength=3.0, max_radius=8):
    """Random t over six octaves, a third of the pixels misses, random radii through strength: a depth edge at every pixel."""
    rng = np.random.default_rng(seed)
    prim = rng.integers(0, 1000, (h, w)).astype(np.uint32)
    prim[rng.random((h, w)) < 1 / 3] = fr.MISS
    pos = np.zeros((h, w, 4), np.float32)
    pos[..., 3] = np.exp2(rng.uniform(-3, 3, (h, w))).astype(np.float32)
    pos[prim == fr.MISS, 3] = -1.0
    color = rng.uniform(0, 8, (h, w, 4)).astype(np.float32)
    return dict(prim=prim, position=pos), color, fixed(focus_distance=1.0, strength=strength, max_radius=max_radius)


def test_the_running_sums_are_in_visiting_order():
    gb, color, d = random_scene(23, 19, 1, max_radius=5)
    o = fr.focus(None, gb, (0, 0), color, d, fr.new_state())
    assert o["acted"].any() and (o["covering"] > 20).any() and (o["covering"] < 12).any()
    differs = 0
    for y in range(0, 19, 3):
        for x in range(0, 23, 2):
            want = scalar_pixel(color, o["coc"], o["tp"], 5, x, y)
            assert u32bits(want).tolist() == u32bits(o["color"][y, x, :3]).tolist(), (x, y)
            differs += u32bits(scalar_pixel(color, o["coc"], o["tp"], 5, x, y, reverse=True)).tolist() != u32bits(want).tolist()
    assert differs > 10                                                # the order matters on these inputs


def test_the_square_of_the_float_below_an_integer_stays_below_its_square():
    """What the tile-wise loop bound rests on: e <= fl(m + 0.5) < N = floor(fl(m + 0.5)) + 1 gives fl(e * e) < N * N, so no tap with
    |dx| or |dy| >= N covers.  And fl(m + 0.5) reaches 1 already at m = the float below 0.5: `m < 0.5` is NOT the copy test."""
    for N in range(1, 10):
        e = np.nextafter(f32(N), f32(0))
        assert f32(e * e) < f32(N * N)
    m = np.nextafter(f32(0.5), f32(0))
    assert m < f32(0.5) and f32(m + f32(0.5)) == f32(1.0)
    gb = plane(5, 5, 1.0)
    gb["prim"][:] = fr.MISS                                            # i = 0 on a miss: r = strength * D
    color = np.random.default_rng(0).uniform(0, 1, (5, 5, 4)).astype(np.float32)
    d = fixed(focus_distance=1.0, strength=float(m), max_radius=2)
    o = fr.focus(None, gb, (0, 0), color, d, fr.new_state())
    assert (o["coc"] == m).all() and o["covering"][2, 2] == 5          # e = 1: the four direct neighbours cover
    assert (fr.tile_bounds(o["coc"], 2) == 1).all()


@pytest.mark.parametrize("case", ["random", "quiet tiles", "below a half", "small radii"])
def test_the_kernels_shortcuts_change_no_bit(case):
    w, h = 70, 37                                                      # three by three tiles of 32 x 16, the last ones partial
    if case == "random":
        gb, color, d = random_scene(w, h, 2)
    elif case == "small radii":
        gb, color, d = random_scene(w, h, 3, strength=0.4, max_radius=6)
    else:
        gb, color, d = random_scene(w, h, 4, strength=0.0 if case == "quiet tiles" else float(np.nextafter(f32(0.5), f32(0))))
        if case == "quiet tiles":                                      # everything in focus but one blurred corner
            d["strength"] = 2.0
            gb["prim"][:] = 1
            gb["position"][..., 3] = 1.0
            gb["position"][30:, 60:, 3] = 0.25
    o = fr.focus(None, gb, (0, 0), color, d, fr.new_state())
    bound = fr.tile_bounds(o["coc"], d["max_radius"])
    short, covering, _, _ = fr.gather(color, o["coc"], o["tp"], d["max_radius"], bound)
    short[bound == 0] = color[bound == 0]                              # the tile copy
    assert np.array_equal(u32bits(short), u32bits(o["color"])) and np.array_equal(covering[bound > 0], o["covering"][bound > 0])
    assert (o["covering"][bound == 0] == 1).all()
    if case == "quiet tiles":
        assert (bound == 0).any() and (bound > 0).any() and (o["covering"] > 1).any()
    if case == "small radii":
        assert 0 < bound.max() < d["max_radius"] and (o["covering"] > 1).any()
    if case == "random":
        assert (bound == d["max_radius"]).all()


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_mirrors_have_the_documented_sizes():
    assert (C.sizeof(abi.FocusConfig), C.sizeof(abi.FocusState)) == (64, 32)
    assert abi.FocusConfig.strength.offset == 16 and abi.FocusConfig._reserved.offset == 36 and abi.FocusState.count.offset == 16


def test_focus_defaults_are_the_documented_ones(so):
    d = abi.FocusConfig()
    C.memset(C.byref(d), 0xff, C.sizeof(d))
    assert so.fovpt_focus_defaults(C.byref(d)) == 0
    assert d.as_dict() == fr.DEFAULTS and list(d._reserved) == [0] * 7
    assert (d.mode, d.meter_radius, d.rank_permille, d.max_radius, d.strength) == (abi.FOCUS_AUTO, 12, 250, 6, 8.0)
    assert so.fovpt_focus_defaults(None) == -1
    assert (abi.FOCUS_FIXED, abi.FOCUS_AUTO, abi.FOCUS_MAX_RADIUS, abi.FOCUS_MAX_METER_RADIUS, abi.FOCUS_BINS) == \
           (fr.FIXED, fr.AUTO, fr.MAX_RADIUS, fr.MAX_METER_RADIUS, fr.BINS) == (0, 1, 8, 64, 256)


def test_focus_rejects_what_needs_no_device(so):
    d, lp, s, g = abi.FocusConfig(), abi.LaunchParams(), abi.FocusState(), abi.GBufferPtrs()
    so.fovpt_focus_defaults(C.byref(d))
    assert so.fovpt_focus(None, C.byref(lp), C.byref(d), None, None, None, None, None) == -1
    assert so.fovpt_focus(None, C.byref(lp), C.byref(d), C.byref(g), None, None, None, None) == -1
    col, rgba = C.c_void_p(), C.c_void_p()
    assert so.fovpt_focus_buffers(None, C.byref(col), C.byref(rgba)) == -1
    assert so.fovpt_focus_state(None, C.byref(s)) == -1 and so.fovpt_focus_reset(None) == -1


def _args(hdr, name):
    m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
    assert m, "fovpt.h does not declare %s" % name
    return [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", a).strip()) for a in m.group(1).replace("\n", " ").split(",")]


def test_the_prototypes_agree_everywhere(so):
    hdr = open(os.path.join(ROOT, "include", "fovpt.h")).read()
    assert _args(hdr, "fovpt_focus_defaults") == ["fovpt_focus_config* out"]
    assert _args(hdr, "fovpt_focus") == ["fovpt_ctx* ctx", "const fovpt_launch_params* lp", "const fovpt_focus_config* fc",
                                         "const fovpt_gbuffer_ptrs* gbuffer", "const fovpt_float4* in_color", "fovpt_float4* out_color",
                                         "uint32_t* out_rgba", "float* out_coc"]
    assert _args(hdr, "fovpt_focus_buffers") == ["fovpt_ctx* ctx", "fovpt_float4** color", "uint32_t** rgba"]
    assert _args(hdr, "fovpt_focus_state") == ["fovpt_ctx* ctx", "struct fovpt_focus_state* out"]
    assert _args(hdr, "fovpt_focus_reset") == ["fovpt_ctx* ctx"]
    for name, value in (("FOCUS_FIXED", 0), ("FOCUS_AUTO", 1), ("FOCUS_MAX_RADIUS", 8), ("FOCUS_MAX_METER_RADIUS", 64), ("FOCUS_BINS", 256)):
        assert re.search(r"#define FOVPT_%s\s+%d\b" % (name, value), hdr)
        assert getattr(abi, name) == value
    vp = C.c_void_p
    assert list(so.fovpt_focus.argtypes) == [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.FocusConfig), C.POINTER(abi.GBufferPtrs), vp, vp, vp, vp]
    assert list(so.fovpt_focus_state.argtypes) == [vp, C.POINTER(abi.FocusState)]
    names = subprocess.check_output(["nm", "-D", "--defined-only", lib.SO_PATH], text=True)
    for sym in ("fovpt_focus_defaults", "fovpt_focus", "fovpt_focus_buffers", "fovpt_focus_state", "fovpt_focus_reset"):
        assert re.search(r"\bT %s\b" % sym, names), sym
        assert getattr(so, sym).restype == C.c_int and sym in lib.EXPORTS
    kernels = subprocess.check_output(["strings", lib.SO_PATH], text=True)
    for k in ("k_focus_meter", "k_focus_radius", "k_focus_gather"):
        assert k in kernels, k


def test_the_struct_mirrors_match_the_header():
    for ctype, mirror, size in (("fovpt_focus_config", abi.FocusConfig, 64), ("struct fovpt_focus_state", abi.FocusState, 32)):
        names = [f[0] for f in mirror._fields_]
        got = header_layout.layout(ctype, mirror)
        assert got[0] == C.sizeof(mirror) == size
        assert got[1:] == [getattr(mirror, n).offset for n in names]


def test_the_static_asserts_compile():
    src = '#include <cstddef>\n#include "fovpt.h"\nstatic_assert(sizeof(fovpt_focus_config) == 64, "config");\n' \
          'static_assert(sizeof(struct fovpt_focus_state) == 32, "state");\n' \
          'int f(fovpt_ctx* c) { struct fovpt_focus_state s; return fovpt_focus_state(c, &s); }\n'
    header_layout.syntax_check(src)
    hdr = open(os.path.join(ROOT, "include", "fovpt.h")).read()
    for name in ("fovpt_focus_config", "struct fovpt_focus_state"):
        assert re.search(r"static_assert\(sizeof\(%s\) == " % re.escape(name), hdr), name


def test_the_dropin_header_compiles():
    src = '#include "SimplePathtracer.h"\nvoid f(SampleRenderer& s, fovpt_float4* c, uint32_t* h) { s.focus(); s.focus(true); ' \
          'fovpt_focus_config fc; fovpt_focus_defaults(&fc); fc.mode = FOVPT_FOCUS_FIXED; fc.max_radius = FOVPT_FOCUS_MAX_RADIUS; ' \
          'fc.strength = s.focusStrength(0.05f); s.focus(fc); s.focus(fc, true, c); s.focusPost(fc); struct fovpt_focus_state st = s.focusState(); ' \
          '(void)st.focus; s.focusReset(); s.downloadFocus(c, h); }\n'
    header_layout.syntax_check(src)


def test_focus_strength_is_the_thin_lens_factor():
    """renderer.focus_strength: lens_radius * (h / 2) * |W| / |V| of the current camera (host only: no context is touched)."""
    from fovpathtracing_optixcodelatest_amd import renderer

    class Stub:
        launchParams = abi.LaunchParams()
    s = Stub()
    s.launchParams.frame.size.y = 1080
    s.launchParams.camera.V.set((0.0, 0.5, 0.0))
    s.launchParams.camera.W.set((0.0, 3.0, 4.0))
    assert renderer.SampleRenderer.focus_strength(s, 0.02) == pytest.approx(0.02 * 540 * 5.0 / 0.5, rel=1e-6)
