"""fovpt_warp without a GPU: the restatement (tests/warp_ref.py) on hand-built G-buffers -- a wall, a smaller face in front of it
and sky around, and a few source pixels placed by hand --, the defaults through ctypes, the struct mirrors against the header,
the prototypes and the C++ drop-in."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import header_layout
import warp_ref as wr
from fovpathtracing_optixcodelatest_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
W, H = 193, 109
AXES = dict(U=(0.75, 0.0, 0.0), V=(0.0, 0.42, 0.0), W=(0.0, 0.0, -1.0))


@pytest.fixture(scope="module")
def so():
    lib.build()
    return lib.load()


def camera(eye=(0.0, 0.0, 0.0), turn=0.0):
    """The scene's camera at eye, turned by `turn` radians about the y axis."""
    c, s = np.cos(turn), np.sin(turn)
    rot = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return dict(eye=tuple(f32(v) for v in eye), **{k: tuple(f32(x) for x in rot @ np.array(v)) for k, v in AXES.items()})


def wall_scene(w=W, h=H):
    """The G-buffer camera() sees: a wall at z = -10 (|x| < 6, |y| < 3.4: sky shows around it), a face at z = -4 (|x| < 0.8,
    |y| < 0.6) in front of it.  prim 0: the wall, 1: the face."""
    cam = camera()
    d = wr.tr.miss_dirs(w, h, cam["U"], cam["V"], cam["W"])
    prim = np.full((h, w), wr.MISS, np.uint32)
    pos = np.zeros((h, w, 4), np.float32)
    pos[..., 3] = -1.0
    for k, (z, ex, ey) in enumerate(((-10.0, 6.0, 3.4), (-4.0, 0.8, 0.6))):          # far to near: the nearer overwrites
        t = f32(-z)                                                                   # (d.z is -1)
        X = (d * t).astype(np.float32)
        on = (np.abs(X[..., 0]) < ex) & (np.abs(X[..., 1]) < ey)
        prim[on] = k
        pos[on, :3] = X[on]
        pos[on, 3] = t
    return dict(prim=prim, position=pos), cam


MOTIONS = dict(identity=camera(), slide=camera((0.35, 0.0, 0.0)), dolly_in=camera((0.0, 0.0, -1.5)), dolly_out=camera((0.0, 0.0, 1.5)),
               turn=camera(turn=0.25))


@pytest.fixture(scope="module")
def scene():
    gb, cam = wall_scene()
    rng = np.random.default_rng(2)
    color = rng.uniform(0, 4, (H, W, 4)).astype(np.float32)
    rgba = rng.integers(0, 1 << 32, (H, W), dtype=np.uint64).astype(np.uint32)
    return gb, cam, color, rgba


# ---- the restatement on the wall scene -----------------------------------------------------------------------------------------------
def test_the_scene_has_all_three_surfaces():
    gb, _ = wall_scene()
    n = H * W
    shares = [(gb["prim"] == p).sum() / n for p in (0, 1, wr.MISS)]
    assert all(s > 0.02 for s in shares) and abs(sum(shares) - 1) < 1e-12, shares


def test_identity_is_the_frame_itself(scene):
    gb, cam, color, rgba = scene
    o = wr.warp(gb, cam, MOTIONS["identity"], None, color, rgba)
    q = np.arange(H * W, dtype=np.uint32).reshape(H, W)
    assert np.array_equal(o["map"], q)                                    # class 0 everywhere
    assert o["counts"] == (H * W, H * W, 0, 0)
    assert np.array_equal(o["color"].view(np.uint32), color.view(np.uint32)) and np.array_equal(o["rgba"], rgba)
    assert wr.collisions(o["dest"]).max() == 1


@pytest.mark.parametrize("motion", ["slide", "dolly_in", "dolly_out", "turn"])
def test_the_motions_are_not_vacuous(scene, motion):
    gb, cam, color, rgba = scene
    o = wr.warp(gb, cam, MOTIONS[motion], None, color, rgba)
    n = H * W
    splatted, direct, filled, empty = o["counts"]
    print(motion, "direct %.1f %% filled %.1f %% empty %.1f %% collisions %.1f %%" %
          (100 * direct / n, 100 * filled / n, 100 * empty / n, 100 * (wr.collisions(o["dest"]) >= 2).sum() / n))
    assert direct + filled + empty == n and splatted <= n
    assert direct > n // 2 and filled > 0 and (wr.collisions(o["dest"]) >= 2).any()
    if motion in ("slide", "dolly_out", "turn"):
        assert empty > 0                                                  # the frame's edge has nothing to show
    if motion == "dolly_in":
        assert empty == 0 and splatted == n                               # the sky around the wall stays where it is
    if motion == "turn":
        assert splatted < n                                               # sources leave the frame on one side
    # the outputs are the inputs at the map's sources, and the map's classes are the counts'
    src, cls = o["map"] & np.uint32(0x3fffffff), o["map"] >> np.uint32(30)
    assert np.array_equal(o["rgba"].reshape(-1), rgba.reshape(-1)[src.reshape(-1)])
    assert np.array_equal(o["color"].reshape(-1, 4).view(np.uint32), color.reshape(-1, 4)[src.reshape(-1)].view(np.uint32))
    assert (src[cls == wr.EMPTY] == np.arange(n, dtype=np.uint32).reshape(H, W)[cls == wr.EMPTY]).all()
    assert np.array_equal(cls == wr.DIRECT, o["keys"] != wr.NO_KEY)
    # a direct pixel shows the nearest source that lands on it: no landed source of it has a smaller depth word
    flat = o["dest"].reshape(-1)
    on = flat >= 0
    nearest = np.full(n, 0xffffffff, np.uint64)
    np.minimum.at(nearest, flat[on], o["depth"].reshape(-1)[on].astype(np.uint64))
    have = o["keys"].reshape(-1) != wr.NO_KEY
    assert np.array_equal((o["keys"].reshape(-1) >> np.uint64(32))[have], nearest[have]) and np.array_equal(have, nearest != 0xffffffff)


def test_the_face_occludes_the_wall_it_slides_over(scene):
    """slide: the camera moves right, so the near face moves left over wall pixels: where a face source and a wall source land
    on one pixel the face wins, also where its index is the higher one; the wall the face uncovers is filled ring by ring."""
    gb, cam, color, rgba = scene
    o = wr.warp(gb, cam, MOTIONS["slide"], None, color, rgba)
    prim, d = gb["prim"].reshape(-1), o["dest"].reshape(-1)
    both = np.zeros(H * W, np.int64)
    for p, bit in ((0, 1), (1, 2)):
        on = (prim == p) & (d >= 0)
        np.bitwise_or.at(both, d[on], bit)
    contested = both == 3
    src = (o["map"] & np.uint32(0x3fffffff)).reshape(-1)
    assert contested.sum() > 20 and (prim[src[contested]] == 1).all()
    assert wr.winner_is_not_lowest(o["dest"], o["keys"])[contested].any()
    filled = ((o["map"] >> np.uint32(30)) == wr.FILLED).reshape(-1)
    hole = filled & (np.abs(np.arange(H * W) % W - W // 2) < W // 4) & (np.abs(np.arange(H * W) // W - H // 2) < H // 8)      # beside the face
    # the hole the face leaves is wider than two rings: its face side is filled from the face, its wall side from the wall, and a
    # hole pixel with a wall key in its first ring takes the wall whatever else the ring holds (the farthest key of the ring)
    assert hole.sum() > 20 and set(prim[src[hole]].tolist()) == {0, 1}
    cls = (o["map"] >> np.uint32(30)).reshape(-1)
    beside_wall = np.flatnonzero(hole)
    beside_wall = beside_wall[(cls[beside_wall + 1] == wr.DIRECT) & (prim[src[beside_wall + 1]] == 0)]
    assert len(beside_wall) > 5 and (prim[src[beside_wall]] == 0).all()


# ---- source pixels placed by hand ----------------------------------------------------------------------------------------------------
def strip(points, w=8):
    """A w x 1 frame seen by the camera U = x, V = y, W = -z at the origin, warped to the same camera: points maps a source pixel
    to its position (None: a miss); the other pixels are hits far outside the frame."""
    cam = dict(eye=(0, 0, 0), U=(1, 0, 0), V=(0, 1, 0), W=(0, 0, -1))
    prim = np.zeros((1, w), np.uint32)
    pos = np.zeros((1, w, 4), np.float32)
    pos[..., :3] = (50.0, 0.0, -1.0)
    for s, p in points.items():
        if p is None:
            prim[0, s] = wr.MISS
        else:
            pos[0, s, :3] = p
    return dict(prim=prim, position=pos), cam


def at(px, z, w=8):
    """A point at depth z that projects onto pixel coordinate px of the strip."""
    return ((2.0 * (px + 0.5) / w - 1.0) * z, 0.0, -z)


def test_the_depth_test_ignores_the_index_order():
    # two hits on pixel 4: the nearer one wins, with the lower index and with the higher
    for near, far in ((2, 5), (5, 2)):
        gb, cam = strip({near: at(4.1, 4.0), far: at(3.9, 10.0)})
        o = wr.warp(gb, cam, cam, dict(fill_radius=0), np.zeros((1, 8, 4), np.float32), np.arange(8, dtype=np.uint32)[None])
        assert o["dest"].reshape(-1).tolist() == [-1, -1, 4, -1, -1, 4, -1, -1]
        assert o["map"][0, 4] == near and o["rgba"][0, 4] == near and o["counts"] == (2, 1, 0, 7)
    # a hit and a miss (pixel 4's own ray lands on pixel 4): the hit wins whatever its depth and index
    for hit in (1, 6):
        gb, cam = strip({4: None, hit: at(4.2, 1e30)})
        o = wr.warp(gb, cam, cam, dict(fill_radius=0), np.zeros((1, 8, 4), np.float32), np.arange(8, dtype=np.uint32)[None])
        assert wr.collisions(o["dest"])[4] == 2 and o["map"][0, 4] == hit
        assert o["keys"][0, 4] >> np.uint64(32) == f32(1e30).view(np.uint32)
    # the miss alone: the sky's depth word
    gb, cam = strip({4: None})
    o = wr.warp(gb, cam, cam, dict(fill_radius=0), np.zeros((1, 8, 4), np.float32), np.arange(8, dtype=np.uint32)[None])
    assert o["keys"][0, 4] == (np.uint64(0x7fffffff) << np.uint64(32)) | np.uint64(4) and o["counts"] == (1, 1, 0, 7)


def test_equal_depths_go_to_the_lower_index():
    gb, cam = strip({6: at(3.8, 10.0), 1: at(4.3, 10.0), 3: at(4.0, 10.0)})
    o = wr.warp(gb, cam, cam, dict(fill_radius=0), np.zeros((1, 8, 4), np.float32), np.arange(8, dtype=np.uint32)[None])
    assert wr.collisions(o["dest"])[4] == 3 and len(set(o["depth"].reshape(-1)[[1, 3, 6]].tolist())) == 1
    assert o["map"][0, 4] == 1


def test_rejected_sources_land_nowhere():
    nan = float("nan")
    gb, cam = strip({0: (0.0, 0.0, 5.0), 1: (0.0, 0.0, 0.0), 2: (nan, 0.0, -3.0), 3: (0.0, nan, -3.0), 4: (0.0, 0.0, nan),
                     5: (float("inf"), 0.0, -3.0), 6: at(8.0, 3.0), 7: at(-0.6, 3.0)})
    dest, _ = wr.landing(gb, cam, cam)
    assert (dest == -1).all()
    o = wr.warp(gb, cam, cam, dict(fill_radius=4), np.ones((1, 8, 4), np.float32), np.arange(8, dtype=np.uint32)[None])
    assert o["counts"] == (0, 0, 0, 8) and np.array_equal(o["map"][0], np.arange(8, dtype=np.uint32) | np.uint32(2 << 30))
    # the frame's edges: -0.5 <= px < w - 0.5 lands
    gb, cam = strip({0: at(7.49, 3.0), 1: at(-0.49, 3.0)})
    assert wr.landing(gb, cam, cam)[0].reshape(-1)[:2].tolist() == [7, 0]
    # a singular camera is the library's to refuse
    assert wr.landing(gb, cam, dict(cam, W=(0, 0, 0))) is None


def key(depth, s):
    return (np.uint64(f32(depth).view(np.uint32)) << np.uint64(32)) | np.uint64(s)


def test_the_ring_rule():
    keys = np.full((9, 9), wr.NO_KEY, np.uint64)
    keys[4, 5] = key(2.0, 40)                                             # r = 1 of (4, 4): near
    keys[4, 6] = key(9.0, 41)                                             # r = 2 of (4, 4): far
    keys[2, 2] = key(5.0, 42)                                             # r = 2 of (4, 4), r = 1 of (3, 3)
    for R in range(5):
        src, cls = wr.resolve(keys, R)
        assert (cls[keys != wr.NO_KEY] == wr.DIRECT).all()
        if R == 0:
            assert (cls[keys == wr.NO_KEY] == wr.EMPTY).all() and src[4, 4] == 4 * 9 + 4      # nothing is filled
            continue
        assert (cls[4, 4], src[4, 4]) == (wr.FILLED, 40)                  # the smallest ring ends the search: the near key
        assert (cls[3, 3], src[3, 3]) == (wr.FILLED, 42)
        assert (cls[4, 8], src[4, 8]) == ((wr.FILLED, 41) if R >= 2 else (wr.EMPTY, 4 * 9 + 8))
        assert cls[8, 0] == wr.EMPTY and src[8, 0] == 8 * 9                    # (8, 0) is 5 or more away from every key
    # within a ring the farthest key wins; equal depths: the larger key, the higher index
    keys = np.full((5, 5), wr.NO_KEY, np.uint64)
    keys[1, 1], keys[1, 3], keys[3, 2] = key(3.0, 7), key(8.0, 3), key(5.0, 20)
    src, cls = wr.resolve(keys, 1)
    assert (cls[2, 2], src[2, 2]) == (wr.FILLED, 3)
    keys[3, 3] = key(8.0, 4)
    assert wr.resolve(keys, 1)[0][2, 2] == 4
    # the sky is the farthest of all
    keys[2, 1] = (np.uint64(0x7fffffff) << np.uint64(32)) | np.uint64(11)
    assert wr.resolve(keys, 1)[0][2, 2] == 11
    # a ring is clipped by the frame
    keys = np.full((3, 3), wr.NO_KEY, np.uint64)
    keys[2, 2] = key(1.0, 8)
    src, cls = wr.resolve(keys, 2)
    assert (cls == np.array([[1, 1, 1], [1, 1, 1], [1, 1, 0]])).all() and (src == 8).all()
    assert (wr.resolve(keys, 1)[1] == np.array([[2, 2, 2], [2, 1, 1], [2, 1, 0]])).all()


def test_images_choose_the_outputs(scene):
    gb, cam, color, rgba = scene
    a = wr.warp(gb, cam, MOTIONS["turn"], dict(images=wr.COLOR), color, None)
    b = wr.warp(gb, cam, MOTIONS["turn"], dict(images=wr.RGBA), None, rgba)
    assert a["rgba"] is None and b["color"] is None and np.array_equal(a["map"], b["map"]) and a["counts"] == b["counts"]


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_mirrors_have_the_documented_sizes():
    assert (C.sizeof(abi.WarpCamera), C.sizeof(abi.WarpConfig), C.sizeof(abi.WarpCounts)) == (48, 32, 32)
    assert abi.WarpCamera.W.offset == 36 and abi.WarpConfig.fill_radius.offset == 4 and abi.WarpCounts.direct.offset == 8
    assert abi.LaunchParams.camera.size == 48 and [f[0] for f in abi.WarpCamera._fields_] == ["eye", "U", "V", "W"]


def test_warp_defaults_are_the_documented_ones(so):
    d = abi.WarpConfig()
    C.memset(C.byref(d), 0xff, C.sizeof(d))
    assert so.fovpt_warp_defaults(C.byref(d)) == 0
    assert (d.images, d.fill_radius, list(d._reserved)) == (3, 2, [0] * 6)
    assert d.images == abi.WARP_COLOR | abi.WARP_RGBA and d.as_dict() == wr.DEFAULTS
    assert so.fovpt_warp_defaults(None) == -1
    assert (abi.WARP_COLOR, abi.WARP_RGBA, abi.WARP_MAX_RADIUS) == (wr.COLOR, wr.RGBA, wr.MAX_RADIUS) == (1, 2, 4)
    assert (abi.WARP_DIRECT, abi.WARP_FILLED, abi.WARP_EMPTY) == (wr.DIRECT, wr.FILLED, wr.EMPTY)


def test_warp_rejects_a_null_context(so):
    d, lp, to, n, g = abi.WarpConfig(), abi.LaunchParams(), abi.WarpCamera(), abi.WarpCounts(), abi.GBufferPtrs()
    so.fovpt_warp_defaults(C.byref(d))
    assert so.fovpt_warp(None, C.byref(lp), C.byref(to), C.byref(d), None, None, None, None, None, None) == -1
    col, rgba = C.c_void_p(), C.c_void_p()
    assert so.fovpt_warp_buffers(None, C.byref(col), C.byref(rgba)) == -1
    assert so.fovpt_warp_counts(None, C.byref(n)) == -1 and so.fovpt_temporal_gbuffer(None, C.byref(g)) == -1


def _args(hdr, name):
    m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
    assert m, "fovpt.h does not declare %s" % name
    return [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", a).strip()) for a in m.group(1).replace("\n", " ").split(",")]


def test_the_prototypes_agree_everywhere(so):
    hdr = open(os.path.join(ROOT, "include", "fovpt.h")).read()
    assert _args(hdr, "fovpt_warp_defaults") == ["fovpt_warp_config* out"]
    assert _args(hdr, "fovpt_warp") == ["fovpt_ctx* ctx", "const fovpt_launch_params* lp", "const fovpt_warp_camera* to", "const fovpt_warp_config* wc",
                                        "const fovpt_gbuffer_ptrs* gbuffer", "const fovpt_float4* in_color", "const uint32_t* in_rgba",
                                        "fovpt_float4* out_color", "uint32_t* out_rgba", "uint32_t* out_map"]
    assert _args(hdr, "fovpt_warp_buffers") == ["fovpt_ctx* ctx", "fovpt_float4** color", "uint32_t** rgba"]
    assert _args(hdr, "fovpt_warp_counts") == ["fovpt_ctx* ctx", "struct fovpt_warp_counts* out"]
    assert _args(hdr, "fovpt_temporal_gbuffer") == ["fovpt_ctx* ctx", "fovpt_gbuffer_ptrs* out"]
    for name, value in (("WARP_COLOR", 1), ("WARP_RGBA", 2), ("WARP_MAX_RADIUS", 4)):
        assert re.search(r"#define FOVPT_%s\s+%d\b" % (name, value), hdr)
        assert getattr(abi, name) == value
    vp = C.c_void_p
    assert list(so.fovpt_warp.argtypes) == [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.WarpCamera), C.POINTER(abi.WarpConfig),
                                            C.POINTER(abi.GBufferPtrs), vp, vp, vp, vp, vp]
    assert list(so.fovpt_warp_counts.argtypes) == [vp, C.POINTER(abi.WarpCounts)]
    names = subprocess.check_output(["nm", "-D", "--defined-only", lib.SO_PATH], text=True)
    for sym in ("fovpt_warp_defaults", "fovpt_warp", "fovpt_warp_buffers", "fovpt_warp_counts", "fovpt_temporal_gbuffer"):
        assert re.search(r"\bT %s\b" % sym, names), sym
        assert getattr(so, sym).restype == C.c_int and sym in lib.EXPORTS
    kernels = subprocess.check_output(["strings", lib.SO_PATH], text=True)
    for k in ("k_warp_scatter", "k_warp_resolve"):
        assert k in kernels, k


def test_the_struct_mirrors_match_the_header():
    for ctype, mirror, size in (("fovpt_warp_camera", abi.WarpCamera, 48), ("fovpt_warp_config", abi.WarpConfig, 32),
                                ("struct fovpt_warp_counts", abi.WarpCounts, 32)):
        names = [f[0] for f in mirror._fields_]
        got = header_layout.layout(ctype, mirror)
        assert got[0] == C.sizeof(mirror) == size
        assert got[1:] == [getattr(mirror, n).offset for n in names]


def test_the_static_asserts_compile():
    src = '#include <cstddef>\n#include "fovpt.h"\nstatic_assert(sizeof(fovpt_warp_camera) == 48, "camera");\n' \
          'static_assert(sizeof(fovpt_warp_config) == 32, "config");\nstatic_assert(sizeof(struct fovpt_warp_counts) == 32, "counts");\n' \
          'static_assert(offsetof(fovpt_launch_params, traversable) - offsetof(fovpt_launch_params, camera) >= sizeof(fovpt_warp_camera), "layout");\n' \
          'int f(fovpt_ctx* c) { struct fovpt_warp_counts n; return fovpt_warp_counts(c, &n); }\n'
    header_layout.syntax_check(src)
    hdr = open(os.path.join(ROOT, "include", "fovpt.h")).read()
    for name in ("fovpt_warp_camera", "fovpt_warp_config", "struct fovpt_warp_counts"):
        assert re.search(r"static_assert\(sizeof\(%s\) == " % re.escape(name), hdr), name


def test_the_dropin_header_compiles():
    src = '#include "SimplePathtracer.h"\nvoid f(SampleRenderer& s, const sutil::Camera& to, fovpt_float4* m, uint32_t* h) { s.warp(to); ' \
          'fovpt_warp_config wc; fovpt_warp_defaults(&wc); wc.images = FOVPT_WARP_RGBA; wc.fill_radius = FOVPT_WARP_MAX_RADIUS; ' \
          's.warp(to, wc); s.warp(to, true); s.warp(to, wc, true, m, h); struct fovpt_warp_counts n = s.warpCounts(); (void)n.splatted; ' \
          's.warpExposed(to); s.warpExposed(to, true); s.downloadWarpedPixels(h); }\n'
    header_layout.syntax_check(src)
