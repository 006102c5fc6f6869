"""fovpt_warp_motion without a GPU: the restatement (tests/warp_motion_ref.py) on the hand-built wall scene of test_warp_cpu.py
with the face as the moved mesh -- its reduction to fovpt_warp, a translation that is exact in binary32, non-finite points --,
the defaults through ctypes, the struct mirror against the header, the prototypes and the C++ drop-in."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import header_layout
import warp_motion_ref as wm
import warp_ref as wr
from fovpathtracing_optixcodelatest_amd import abi, lib

from test_warp_cpu import H, MOTIONS, W, _args, camera, strip, wall_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SHIFT = np.array([0.25, 0.0625, 0.0], np.float32)          # the face's move per step: exact in binary32, 8 px and 2 px at its depth
# the face (prim 1) as one triangle that covers it, a = (-1, -1, -4), b = (3, -1, -4), c = (-1, 3, -4): u = (x + 1) / 4, v = (y + 1) / 4
FACE = np.array([[-1.0, -1.0, -4.0], [3.0, -1.0, -4.0], [-1.0, 3.0, -4.0]], np.float32)
WALL = np.array([[-20.0, -20.0, -10.0], [40.0, -20.0, -10.0], [-20.0, 40.0, -10.0]], np.float32)


@pytest.fixture(scope="module")
def so():
    lib.build()
    return lib.load()


def face_motion(moved=True, shift=SHIFT):
    """The dict MotionChecker.motion() makes, for the wall scene: mesh 0 the wall, mesh 1 the face, which was at -shift when the
    interval began."""
    vtx = np.concatenate([WALL, FACE])
    prev = vtx.copy()
    prev[3:] = FACE - shift
    return dict(tri_vidx=np.array([[0, 1, 2], [3, 4, 5]]), vtx_prev=prev, vtx=vtx, mesh_of_prim=np.array([0, 1]), moved=np.array([False, moved]))


@pytest.fixture(scope="module")
def scene():
    gb, cam = wall_scene()
    X = gb["position"]
    uv = np.zeros((H, W, 2), np.float32)
    face = gb["prim"] == 1
    uv[face, 0] = (X[face, 0] + f32(1.0)) * f32(0.25)
    uv[face, 1] = (X[face, 1] + f32(1.0)) * f32(0.25)
    rng = np.random.default_rng(5)
    color = rng.uniform(0, 4, (H, W, 4)).astype(np.float32)
    rgba = rng.integers(0, 1 << 32, (H, W), dtype=np.uint64).astype(np.uint32)
    return gb, uv, cam, color, rgba


def same(a, b):
    assert np.array_equal(a["map"], b["map"]) and a["counts"] == b["counts"] and np.array_equal(a["keys"], b["keys"])
    assert np.array_equal(a["color"].view(np.uint32), b["color"].view(np.uint32)) and np.array_equal(a["rgba"], b["rgba"])


# ---- the restatement on the wall scene -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("motion", ["identity", "slide", "turn"])
def test_it_reduces_to_fovpt_warp(scene, motion):
    gb, uv, cam, color, rgba = scene
    plain = wr.warp(gb, cam, MOTIONS[motion], None, color, rgba)
    same(wm.warp(gb, uv, face_motion(), cam, MOTIONS[motion], dict(advance=0.0), color, rgba), plain)
    for advance in (0.5, 1.0, 4.0):
        same(wm.warp(gb, uv, face_motion(moved=False), cam, MOTIONS[motion], dict(advance=advance), color, rgba), plain)
        same(wm.warp(gb, uv, None, cam, MOTIONS[motion], dict(advance=advance), color, rgba), plain)
    # and a moved face does change it
    assert not np.array_equal(wm.warp(gb, uv, face_motion(), cam, MOTIONS[motion], None, color, rgba)["map"], plain["map"])
    assert wm.extrapolate(gb, uv, face_motion(), 0.0) is gb and wm.extrapolate(gb, uv, face_motion(moved=False), 1.0) is gb


@pytest.mark.parametrize("motion", ["identity", "slide", "turn"])
def test_a_translated_face_lands_where_the_next_translation_puts_it(scene, motion):
    gb, uv, cam, color, rgba = scene
    face = gb["prim"] == 1
    n_face = int(face.sum())
    o = wm.warp(gb, uv, face_motion(), cam, MOTIONS[motion], dict(advance=1.0), color, rgba)
    plain = wr.warp(gb, cam, MOTIONS[motion], None, color, rgba)
    # the face translated once more: its points moved by the step's shift
    nxt = dict(gb, position=gb["position"].copy())
    nxt["position"][face, :3] = gb["position"][face, :3] + SHIFT
    want_dest, _ = wr.landing(nxt, cam, MOTIONS[motion])
    assert np.array_equal(o["dest"][face], want_dest[face]) and (o["dest"][face] >= 0).all()
    assert np.array_equal(o["dest"][~face], plain["dest"][~face])
    differ = int((o["map"] != plain["map"]).sum())
    collide = int((wr.collisions(o["dest"]) >= 2).sum())
    print(motion, "face pixels", n_face, "counts", o["counts"], "collision pixels", collide, "map differences", differ)
    assert n_face > 1000 and differ >= n_face
    assert o["counts"][2] > 0 and collide > 0
    if motion == "identity":
        # the strip the face vacates is 8 px wide: wider than two rings, so its middle stays empty and shows the face's old image
        assert o["counts"][3] > 0
        empty = (o["map"] >> np.uint32(30)) == wr.EMPTY
        assert (empty & face).sum() == o["counts"][3]
        assert wr.warp(gb, cam, MOTIONS[motion], None, color, rgba)["counts"][3] == 0
    # where the face lands it wins over the wall behind it
    src = (o["map"] & np.uint32(0x3fffffff)).reshape(-1)
    landed = np.unique(o["dest"][face])
    assert (gb["prim"].reshape(-1)[src[landed]] == 1).all()


def test_advance_scales_the_displacement(scene):
    gb, uv, cam, _, _ = scene
    face = gb["prim"] == 1
    for advance in (0.5, 2.0, 4.0):
        g2 = wm.extrapolate(gb, uv, face_motion(), advance)
        assert np.array_equal(g2["prim"], gb["prim"]) and np.array_equal(g2["position"][~face], gb["position"][~face])
        assert np.array_equal(g2["position"][..., 3], gb["position"][..., 3])                 # t stays
        d = g2["position"][face, :3].astype(np.float64) - gb["position"][face, :3]
        assert np.abs(d - advance * SHIFT.astype(np.float64)).max() < 1e-5


def test_a_non_finite_point_lands_nowhere():
    nan, inf = float("nan"), float("inf")
    z = 3.0
    at = lambda px: ((2.0 * (px + 0.5) / 8 - 1.0) * z, 0.0, -z)
    gb, cam = strip({k: at(k) for k in range(8)})
    uv = np.zeros((1, 8, 2), np.float32)
    uv[0, :, 0] = np.arange(8) / 8.0
    tri = np.array([at(0), at(8), (at(0)[0], 1.0, -z)], np.float32)
    gb["prim"][0] = np.arange(8)
    prev = np.tile(tri, (8, 1, 1))
    prev[1, 0, 0] = nan                                      # X' is NaN
    prev[2, 1, 1] = inf                                      # X'.y is infinite: d and X* are
    prev[3, 0] = (3e38, 0.0, -z)                             # finite, but advance * d overflows
    prev[4, 2, 2] = -inf                                     # weight 0 times inf: NaN
    prev[5, 1, 2] = nan
    motion = dict(tri_vidx=np.arange(24).reshape(8, 3), vtx_prev=prev.reshape(24, 3), vtx=np.tile(tri, (8, 1)), mesh_of_prim=np.arange(8),
                  moved=np.array([True] * 6 + [False, True]))
    g2 = wm.extrapolate(gb, uv, motion, 4.0)
    assert not np.isfinite(g2["position"][0, 1:6, :3]).all(axis=1).any()
    assert np.isfinite(g2["position"][0, [0, 6, 7], :3]).all()
    o = wm.warp(gb, uv, motion, cam, cam, dict(advance=4.0, fill_radius=0), np.zeros((1, 8, 4), np.float32), np.arange(8, dtype=np.uint32)[None])
    assert o["dest"].reshape(-1).tolist() == [0, -1, -1, -1, -1, -1, 6, 7]
    assert o["counts"] == (3, 3, 0, 5)
    # the same sources land under fovpt_warp: the rejection is the extrapolated point's
    assert wr.warp(gb, cam, cam, dict(fill_radius=0), np.zeros((1, 8, 4), np.float32), np.arange(8, dtype=np.uint32)[None])["counts"] == (8, 8, 0, 0)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_mirror_has_the_documented_size():
    assert C.sizeof(abi.WarpMotionConfig) == 32
    assert [(f[0], getattr(abi.WarpMotionConfig, f[0]).offset) for f in abi.WarpMotionConfig._fields_] == \
        [("images", 0), ("fill_radius", 4), ("advance", 8), ("_reserved", 12)]
    assert abi.WARP_MAX_ADVANCE == wm.MAX_ADVANCE == 4.0


def test_warp_motion_defaults_are_the_documented_ones(so):
    d = abi.WarpMotionConfig()
    C.memset(C.byref(d), 0xff, C.sizeof(d))
    assert so.fovpt_warp_motion_defaults(C.byref(d)) == 0
    assert (d.images, d.fill_radius, d.advance, list(d._reserved)) == (3, 2, 1.0, [0] * 5)
    assert d.as_dict() == wm.DEFAULTS
    assert so.fovpt_warp_motion_defaults(None) == -1


def test_warp_motion_rejects_a_null_context(so):
    d, lp, to = abi.WarpMotionConfig(), abi.LaunchParams(), abi.WarpCamera()
    so.fovpt_warp_motion_defaults(C.byref(d))
    assert so.fovpt_warp_motion(None, C.byref(lp), C.byref(to), C.byref(d), None, None, None, None, None, None) == -1


def test_the_prototypes_agree_everywhere(so):
    hdr = open(os.path.join(ROOT, "include", "fovpt.h")).read()
    assert _args(hdr, "fovpt_warp_motion_defaults") == ["fovpt_warp_motion_config* out"]
    assert _args(hdr, "fovpt_warp_motion") == ["fovpt_ctx* ctx", "const fovpt_launch_params* lp", "const fovpt_warp_camera* to",
                                               "const fovpt_warp_motion_config* mc", "const fovpt_gbuffer_ptrs* gbuffer", "const fovpt_float4* in_color",
                                               "const uint32_t* in_rgba", "fovpt_float4* out_color", "uint32_t* out_rgba", "uint32_t* out_map"]
    assert re.search(r"#define FOVPT_WARP_MAX_ADVANCE\s+4\.0f\b", hdr)
    vp = C.c_void_p
    assert list(so.fovpt_warp_motion_defaults.argtypes) == [C.POINTER(abi.WarpMotionConfig)]
    assert list(so.fovpt_warp_motion.argtypes) == [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.WarpCamera), C.POINTER(abi.WarpMotionConfig),
                                                   C.POINTER(abi.GBufferPtrs), vp, vp, vp, vp, vp]
    names = subprocess.check_output(["nm", "-D", "--defined-only", lib.SO_PATH], text=True)
    for sym in ("fovpt_warp_motion_defaults", "fovpt_warp_motion"):
        assert re.search(r"\bT %s\b" % sym, names), sym
        assert getattr(so, sym).restype == C.c_int and sym in lib.EXPORTS
    assert "k_warp_scatter_motion" in subprocess.check_output(["strings", lib.SO_PATH], text=True)


def test_the_struct_mirror_matches_the_header():
    names = [f[0] for f in abi.WarpMotionConfig._fields_]
    (lay,), consts = header_layout.probe([("fovpt_warp_motion_config", abi.WarpMotionConfig)], ("FOVPT_WARP_MAX_ADVANCE",))
    got = lay + consts
    assert int(got[0]) == C.sizeof(abi.WarpMotionConfig) == 32
    assert [int(x) for x in got[1:-1]] == [getattr(abi.WarpMotionConfig, n).offset for n in names] == [0, 4, 8, 12]
    assert float(got[-1]) == abi.WARP_MAX_ADVANCE


def test_the_static_assert_compiles():
    src = '#include <cstddef>\n#include "fovpt.h"\nstatic_assert(sizeof(fovpt_warp_motion_config) == 32, "config");\n' \
          'static_assert(sizeof(fovpt_warp_motion_config) == sizeof(fovpt_warp_config), "the two configs");\n'
    header_layout.syntax_check(src)
    hdr = open(os.path.join(ROOT, "include", "fovpt.h")).read()
    assert re.search(r"static_assert\(sizeof\(fovpt_warp_motion_config\) == 32", hdr)


def test_the_dropin_header_compiles():
    src = '#include "SimplePathtracer.h"\nvoid f(SampleRenderer& s, const sutil::Camera& to, fovpt_float4* m, uint32_t* h) { s.warpMotion(to, 1.0f); ' \
          'fovpt_warp_motion_config mc; fovpt_warp_motion_defaults(&mc); mc.images = FOVPT_WARP_RGBA; mc.advance = FOVPT_WARP_MAX_ADVANCE; ' \
          's.warpMotion(to, mc); s.warpMotion(to, 0.5f, true); s.warpMotion(to, mc, true, m, h); s.warpMotion(to, 2.0f, false, m, h); ' \
          's.warpMotionExposed(to, 1.0f); s.warpMotionExposed(to, 1.5f, true); struct fovpt_warp_counts n = s.warpCounts(); (void)n.filled; ' \
          's.downloadWarpedPixels(h); s.warp(to); s.lens(&to); }\n'
    header_layout.syntax_check(src)
