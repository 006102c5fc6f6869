"""fovpt_temporal_motion without a GPU: its prototype in the header, the ctypes mirror and the C++ drop-in, null arguments, and
properties of the definition, the numpy restatement in tests/temporal_motion_ref.py that the GPU kernel is checked against."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import header_layout
import temporal_motion_ref as tm
import temporal_ref as tr
from fovpathtracing_optixcodelatest_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def so():
    lib.build()
    return lib.load()


def test_the_prototype_agrees_everywhere(so):
    hdr = open(os.path.join(ROOT, "include", "fovpt.h")).read()
    m = re.search(r"int fovpt_temporal_motion\(([^;]*)\);", hdr)
    assert m, "fovpt.h does not declare fovpt_temporal_motion"
    args = [re.sub(r"/\*.*?\*/", "", a).strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert [re.sub(r"\s+", " ", a) for a in args] == [
        "fovpt_ctx* ctx", "const fovpt_launch_params* lp", "const fovpt_temporal_config* tc", "const fovpt_float4* in_color",
        "fovpt_float4* out_color", "uint32_t* out_rgba", "fovpt_float4* out_motion"]
    vp = C.c_void_p
    assert list(so.fovpt_temporal_motion.argtypes) == [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.TemporalConfig), vp, vp, vp, vp]
    assert so.fovpt_temporal_motion.restype == C.c_int
    # the symbol is exported, and the drop-in header calls it with seven arguments, the motion buffer last
    names = subprocess.check_output(["nm", "-D", "--defined-only", lib.SO_PATH], text=True)
    assert re.search(r"\bT fovpt_temporal_motion\b", names)
    shim = open(os.path.join(ROOT, "include", "SimplePathtracer.h")).read()
    call = re.search(r"fovpt_temporal_motion\((.*?)\)\);", shim, re.S)
    assert call and len(call.group(1).replace("reinterpret_cast<const fovpt_launch_params*>(&launchParams)", "lp").split(",")) == 7
    assert "void temporalMotion(" in shim and "void downloadMotion(" in shim


def test_the_dropin_header_compiles(tmp_path):
    src = '#include "SimplePathtracer.h"\nvoid f(SampleRenderer& s, fovpt_float4* m, float4* h) { s.temporalMotion(); s.temporalMotion(nullptr, m); ' \
          'fovpt_temporal_config tc; fovpt_temporal_defaults(&tc); s.temporalMotion(tc, nullptr, m); s.downloadMotion(m, h); }\n'
    header_layout.syntax_check(src)


def test_temporal_motion_rejects_a_null_context(so):
    d = abi.TemporalConfig()
    so.fovpt_temporal_defaults(C.byref(d))
    lp = abi.LaunchParams()
    assert so.fovpt_temporal_motion(None, C.byref(lp), C.byref(d), None, None, None, None) == -1


# ---- random synthetic G-buffers: without motion the restatement is temporal_ref.step ------------------------------------------
def _random_inputs(seed, w=37, h=23, ntri=40, nmesh=5):
    rng = np.random.default_rng(seed)
    cam = dict(eye=tuple(rng.normal(0, 1, 3)), U=(1.0, 0.0, 0.1), V=(0.0, 0.7, 0.0), W=(0.1, 0.0, 1.0))
    pcam = dict(eye=tuple(rng.normal(0, 1, 3)), U=(1.0, 0.1, 0.0), V=(0.0, 0.8, 0.0), W=(0.0, 0.1, 1.0))

    def gbuffer():
        prim = rng.integers(0, ntri, (h, w)).astype(np.uint32)
        prim[rng.random((h, w)) < 0.2] = tr.MISS
        d = tr.miss_dirs(w, h, cam["U"], cam["V"], cam["W"])
        t = rng.uniform(3, 9, (h, w)).astype(np.float32)
        pos = np.concatenate([np.asarray(cam["eye"], np.float32) + t[..., None] * d, t[..., None]], axis=-1).astype(np.float32)
        n = rng.normal(0, 1, (h, w, 3))
        n = np.where(rng.random((h, w, 1)) < 0.5, (0.0, 0.0, -1.0), n / np.linalg.norm(n, axis=-1, keepdims=True))
        nrm = np.concatenate([n, np.zeros((h, w, 1))], axis=-1).astype(np.float32)
        miss = prim == tr.MISS
        pos[miss], nrm[miss] = (0, 0, 0, -1), 0
        return dict(prim=prim, position=pos, normal=nrm)

    gb, pg = gbuffer(), gbuffer()
    hist = rng.random((h, w, 4), dtype=np.float32)
    hist[..., 3] = rng.integers(1, 6, (h, w))
    inp = rng.random((h, w, 4), dtype=np.float32)
    cap = rng.integers(1, 9, (h, w)).astype(np.int64)
    uv = rng.random((h, w, 2), dtype=np.float32) * f32(0.5)
    vtx = rng.normal(0, 3, (3 * ntri, 3)).astype(np.float32)
    motion = dict(tri_vidx=np.arange(3 * ntri).reshape(ntri, 3), vtx_prev=(vtx + f32(0.25)).astype(np.float32), vtx=vtx,
                  mesh_of_prim=np.sort(rng.integers(0, nmesh, ntri)), moved=np.zeros(nmesh, bool))
    return inp, gb, uv, cap, cam, dict(gb=pg, cam=pcam, history=hist), motion


@pytest.mark.parametrize("seed", range(4))
def test_without_motion_it_is_temporal_ref(seed):
    inp, gb, uv, cap, cam, prev, motion = _random_inputs(seed)
    cfg = dict(normal_tolerance=1.5, depth_tolerance=0.5)
    want = tr.step(inp, gb, cap, cam, prev, cfg)
    assert (want[1][..., 3] > 1).mean() > 0.1                       # (some history is carried: the comparison is not of resets alone)
    for mo in (None, motion):                                        # no motion record; a moved mask that is all false
        out, hist, _ = tm.step(inp, gb, uv, cap, cam, prev, cfg, mo)
        assert np.array_equal(bits(out), bits(want[0])) and np.array_equal(bits(hist), bits(want[1]))
    moved = dict(motion, moved=np.ones(5, bool))                     # (and the mask does matter)
    assert not np.array_equal(bits(tm.step(inp, gb, uv, cap, cam, prev, cfg, moved)[1]), bits(want[1]))
    for p in (None, dict(prev, history=prev["history"][:-1])):       # no history; a history of another size
        out, hist, mv = tm.step(inp, gb, uv, cap, cam, p, cfg, moved)
        assert np.array_equal(bits(out), bits(inp)) and (hist[..., 3] == 1).all() and not mv.any()


# ---- a plane z = 8 of one triangle, facing a still pinhole camera at the origin ------------------------------------------------
# |U| = 1, |V| = 0.5, 16 x 8 pixels: the ray of pixel (x, y) meets the plane at (x + 0.5 - 8, y + 0.5 - 4, 8), one pixel is one
# unit of the plane, and with the triangle's legs 32 long every barycentric and every product below is exact in binary32
W, H, D = 16, 8, 8.0
CAM = dict(eye=(0.0, 0.0, 0.0), U=(1.0, 0.0, 0.0), V=(0.0, 0.5, 0.0), W=(0.0, 0.0, 1.0))
TRI = np.float32([[-8, -4, D], [24, -4, D], [-8, 28, D]])


def _plane(z=D):
    d = tr.miss_dirs(W, H, CAM["U"], CAM["V"], CAM["W"])
    X = (d * f32(z)).astype(np.float32)
    t = np.sqrt((X.astype(np.float64) ** 2).sum(-1)).astype(np.float32)
    nrm = np.zeros((H, W, 4), np.float32)
    nrm[..., 2] = -1.0
    gb = dict(prim=np.zeros((H, W), np.uint32), position=np.concatenate([X, t[..., None]], axis=-1), normal=nrm)
    uv = np.stack([(X[..., 0] + f32(8)) / f32(32), (X[..., 1] + f32(4)) / f32(32)], axis=-1).astype(np.float32)
    return gb, uv


def _history(seed=3):
    h = np.random.default_rng(seed).random((H, W, 4), dtype=np.float32)
    h[..., 3] = 1.0
    return h


def _motion(prev_vertices):
    return dict(tri_vidx=np.array([[0, 1, 2]]), vtx_prev=np.float32(prev_vertices), vtx=TRI, mesh_of_prim=np.array([0]), moved=np.array([True]))


def test_a_plane_moved_by_one_pixel_takes_the_neighbours_history():
    gb, uv = _plane()
    hist, inp, cap = _history(), np.random.default_rng(5).random((H, W, 4), dtype=np.float32), np.full((H, W), 2)
    prev = dict(gb=gb, cam=CAM, history=hist)                        # (a translation inside the plane: the same lattice of points)
    out, h, mv = tm.step(inp, gb, uv, cap, CAM, prev, None, _motion(TRI + f32([1, 0, 0])))   # it came from one unit to the right
    inside = np.s_[:, :-1]
    assert (h[inside][..., 3] == 2).all() and (h[:, -1, 3] == 1).all()            # (the last column came from outside the frame)
    want = hist[:, 1:, :3] + f32(0.5) * (inp[:, :-1, :3] - hist[:, 1:, :3])
    assert np.array_equal(bits(out[inside][..., :3]), bits(want))
    assert np.array_equal(mv[inside][..., :2], np.broadcast_to(f32([1, 0]), (H, W - 1, 2))) and (mv[inside][..., 3] == 1).all()
    assert (mv[inside][..., 2] == f32(D)).all() and not mv[:, -1].any()
    out0, h0 = tr.step(inp, gb, cap, CAM, prev)                      # the camera alone: the pixel's own history
    assert (h0[..., 3] == 2).all()
    assert np.array_equal(bits(out0[..., :3]), bits(hist[..., :3] + f32(0.5) * (inp[..., :3] - hist[..., :3])))


def test_a_plane_pushed_along_its_normal_keeps_its_history():
    gb, uv = _plane()
    pg, _ = _plane(10.0)                                             # where it was: 2 units further, against depth_tolerance * t < 0.5
    assert (tr.DEFAULTS["depth_tolerance"] * gb["position"][..., 3] < 0.5).all()
    prev = dict(gb=pg, cam=CAM, history=_history())
    inp, cap = _history(7), np.full((H, W), 2)
    _, h, mv = tm.step(inp, gb, uv, cap, CAM, prev, None, _motion(TRI + f32([0, 0, 2])))
    assert (np.abs(h[..., 3] - 2) < 1e-5).all() and (mv[..., 2] == f32(10)).all()   # (a bilinear mean of equal lengths may round)
    _, h0 = tr.step(inp, gb, cap, CAM, prev)
    assert (h0[..., 3] == 1).all()


def test_a_zero_area_previous_triangle_starts_a_new_history():
    gb, uv = _plane()
    prev = dict(gb=gb, cam=CAM, history=_history())
    inp, cap = _history(9), np.full((H, W), 2)
    out, h, mv = tm.step(inp, gb, uv, cap, CAM, prev, None, _motion(np.tile(f32([[1, 1, D]]), (3, 1))))
    assert (h[..., 3] == 1).all() and np.array_equal(bits(out), bits(inp))
    assert (mv[..., 3] == 1).all()                                   # (the point itself still projects: only the normal is lost)


def test_motion_out_is_the_projection_minus_the_pixel():
    inp, gb, uv, cap, cam, prev, motion = _random_inputs(11)
    motion = dict(motion, moved=np.array([True, False, True, False, True]))
    _, _, mv = tm.step(inp, gb, uv, cap, cam, None, None, motion)
    assert mv.shape == cap.shape + (4,) and not mv.any()             # no history
    _, _, mv = tm.step(inp, gb, uv, cap, cam, prev, None, motion)
    g2 = tm.substitute(gb, uv, cam, motion)
    px, py, ok = tr.project(g2, cam, prev["cam"])
    y, x = np.mgrid[0:cap.shape[0], 0:cap.shape[1]].astype(np.float32)
    assert 0.1 < ok.mean() < 1.0 and (cap[ok] == 1).any()            # (both kinds of pixel, and cap-1 pixels among the projected)
    assert np.array_equal(mv[..., 3], ok.astype(np.float32)) and not mv[~ok].any()
    assert np.array_equal(bits(mv[ok][:, 0]), bits((px - x)[ok])) and np.array_equal(bits(mv[ok][:, 1]), bits((py - y)[ok]))
    assert (mv[ok][:, 2] > 0).all()
