"""fovpt_temporal without a GPU: the C ABI of its config (layout, defaults, null arguments) and properties of the definition, the
numpy restatement in tests/temporal_ref.py that the GPU kernel is checked against."""
import ctypes as C

import numpy as np
import pytest

import header_layout
import reconstruct_ref as rr
import temporal_ref as tr
from fovpathtracing_optixcodelatest_amd import abi, lib

f32 = np.float32


@pytest.fixture(scope="module")
def so():
    lib.build()
    return lib.load()


def test_struct_mirror_matches_the_header():
    cname, struct = "fovpt_temporal_config", abi.TemporalConfig
    names = [f[0] for f in struct._fields_]
    (lay,), (max_history,) = header_layout.probe([(cname, struct)], ("FOVPT_TEMPORAL_MAX_HISTORY",))
    got = [lay[0], max_history] + lay[1:]
    assert got[0] == C.sizeof(struct) == 32
    assert got[1] == abi.TEMPORAL_MAX_HISTORY == tr.MAX_HISTORY
    assert got[2:] == [getattr(struct, n).offset for n in names]


def test_temporal_defaults_are_documented_and_in_range(so):
    d = abi.TemporalConfig()
    assert so.fovpt_temporal_defaults(C.byref(d)) == 0
    assert d.as_dict() == {k: np.float32(v) if isinstance(v, float) else v for k, v in tr.DEFAULTS.items()}
    for k in ("history_fovea", "history_middle", "history_periphery", "history_uniform"):
        assert 1 <= getattr(d, k) <= abi.TEMPORAL_MAX_HISTORY
    assert 0 <= d.normal_tolerance <= 4 and 0 <= d.depth_tolerance <= 1 and list(d._reserved) == [0, 0]
    assert so.fovpt_temporal_defaults(None) == -1


def test_temporal_rejects_null_arguments(so):
    d = abi.TemporalConfig()
    so.fovpt_temporal_defaults(C.byref(d))
    lp = abi.LaunchParams()
    assert so.fovpt_temporal(None, C.byref(lp), C.byref(d), None, None, None) == -1
    col, rgba, hist = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert so.fovpt_temporal_buffers(None, C.byref(col), C.byref(rgba), C.byref(hist)) == -1
    assert so.fovpt_temporal_reset(None) == -1


# ---- a synthetic scene: axis-aligned rectangles facing -z, a pinhole camera looking along +z ------------------------------
W, H = 64, 48


def _cam(eye, U=(1.0, 0.0, 0.0), V=(0.0, 0.75, 0.0), Wv=(0.0, 0.0, 1.0)):
    return dict(eye=tuple(float(v) for v in eye), U=U, V=V, W=Wv)


def _gbuffer(cam, rects):
    """G-buffer of a camera over rectangles (z, x0, x1, y0, y1), nearest first; normal (0, 0, -1); prim = the rectangle."""
    o, d = rr.primary_rays(W, H, cam["eye"], cam["U"], cam["V"], cam["W"])
    prim = np.full(W * H, tr.MISS, np.uint32)
    pos = np.zeros((W * H, 4), np.float32)
    pos[:, 3] = -1.0
    nrm = np.zeros((W * H, 4), np.float32)
    for k, (z, x0, x1, y0, y1) in reversed(list(enumerate(rects))):
        t = (f32(z) - o[:, 2]) / d[:, 2]
        X = o + t[:, None] * d
        hit = (t > 0) & (X[:, 0] >= x0) & (X[:, 0] <= x1) & (X[:, 1] >= y0) & (X[:, 1] <= y1)
        prim[hit] = k
        pos[hit, :3], pos[hit, 3] = X[hit], t[hit]
        nrm[hit] = (0.0, 0.0, -1.0, 0.0)
    return dict(prim=prim.reshape(H, W), position=pos.reshape(H, W, 4), normal=nrm.reshape(H, W, 4))


def _frame(seed):
    c = np.random.default_rng(seed).random((H, W, 4), dtype=np.float32)
    c[..., 3] = 1.0
    return c


BACK = (10.0, -50.0, 50.0, -50.0, 50.0)


def test_an_identical_camera_reprojects_onto_the_pixel():
    cam = _cam((0.25, -0.5, 0.0))
    for rects in ([BACK], []):                                 # hits, then misses
        gb = _gbuffer(cam, rects)
        px, py, ok = tr.project(gb, cam, cam)
        y, x = np.mgrid[0:H, 0:W].astype(np.float32)
        assert ok.all()
        # one ulp of the frame's extent: the point's rounding in X = eye + t d, then in X - eye and the fp32 inverse
        assert np.abs(px - x).max() <= np.spacing(f32(W)) and np.abs(py - y).max() <= np.spacing(f32(H))


def test_a_one_pixel_shift_takes_the_neighbours_history():
    prev_cam = _cam((0.0, 0.0, 0.0))
    foot = 2.0 * 10.0 / W                                      # one pixel of the plane z = 10 (|U| = 1)
    cam = _cam((-foot, 0.0, 0.0))                              # moved left: the pixel x now sees what x - 1 saw
    pg, gb = _gbuffer(prev_cam, [BACK]), _gbuffer(cam, [BACK])
    hist = np.zeros((H, W, 4), np.float32)
    hist[..., 0] = np.arange(W, dtype=np.float32)[None, :]
    hist[..., 1] = np.arange(H, dtype=np.float32)[:, None]
    hist[..., 3] = 1.0
    cap = np.full((H, W), 8)
    out, h = tr.step(_frame(1), gb, cap, cam, dict(gb=pg, cam=prev_cam, history=hist))
    px, py, _ = tr.project(gb, cam, prev_cam)
    x = np.arange(W)
    assert np.abs(px - (x - 1)[None, :]).max() < 1e-3
    inside = np.s_[:, 1:]
    assert (h[inside][..., 3] == 2.0).all()
    # H = out - (in - out) since out = H + (in - H) / 2
    Hx = 2.0 * out[inside][..., 0].astype(np.float64) - _frame(1)[inside][..., 0]
    assert np.abs(Hx - (x[1:] - 1)[None, :]).max() < 1e-3
    assert (h[:, 0, 3] == 1.0).all()                            # column 0 came from outside the previous frame


def test_uncovered_background_has_no_history():
    prev_cam, cam = _cam((0.0, 0.0, 0.0)), _cam((1.5, 0.0, 0.0))
    front = (5.0, -1.0, 1.0, -1.0, 1.0)
    pg, gb = _gbuffer(prev_cam, [front, BACK]), _gbuffer(cam, [front, BACK])
    hist = np.concatenate([_frame(2)[..., :3], np.ones((H, W, 1), np.float32)], axis=-1)
    out, h = tr.step(_frame(3), gb, np.full((H, W), 8), cam, dict(gb=pg, cam=prev_cam, history=hist))
    # the background pixels whose point is hidden from the previous eye by the front rectangle (segment eye_prev -> X at z = 5)
    X = gb["position"][..., :3].astype(np.float64)
    back = gb["prim"] == 1
    s = (5.0 - 0.0) / X[..., 2]
    xs, ys = X[..., 0] * s, X[..., 1] * s
    hidden = back & (np.abs(xs) < 0.9) & (np.abs(ys) < 0.9)
    seen = back & ((np.abs(xs) > 1.1) | (np.abs(ys) > 1.1))
    assert hidden.sum() > 30 and seen.sum() > 500
    assert (h[hidden][:, 3] == 1.0).all()
    assert np.array_equal(out[hidden].view(np.uint32), _frame(3)[hidden].view(np.uint32))
    px, py, ok = tr.project(gb, cam, prev_cam)
    far = seen & ok & (px > 1) & (px < W - 2) & (py > 1) & (py < H - 2)
    assert far.sum() > 300 and (h[far][:, 3] == 2.0).all()


def test_misses_reproject_by_direction_only():
    prev_cam, cam = _cam((0.0, 0.0, 0.0)), _cam((7.0, -3.0, 2.0))  # a pure translation
    gb, pg = _gbuffer(cam, []), _gbuffer(prev_cam, [])
    hist = np.concatenate([_frame(4)[..., :3], np.full((H, W, 1), 3.0, np.float32)], axis=-1)
    out, h = tr.step(_frame(5), gb, np.full((H, W), 8), cam, dict(gb=pg, cam=prev_cam, history=hist))
    assert (h[..., 3] == 4.0).all()
    assert np.allclose((4.0 * out[..., :3] - _frame(5)[..., :3]) / 3.0, hist[..., :3], atol=1e-5)


def test_a_degenerate_previous_camera_resets_every_pixel():
    cam = _cam((0.0, 0.0, 0.0))
    flat = _cam((0.0, 0.0, 0.0), U=(1.0, 0.0, 0.0), V=(2.0, 0.0, 0.0))
    assert tr.camera_inverse(flat["U"], flat["V"], flat["W"]) is None
    gb = _gbuffer(cam, [BACK])
    hist = np.concatenate([_frame(6)[..., :3], np.ones((H, W, 1), np.float32)], axis=-1)
    inp = _frame(7)
    out, h = tr.step(inp, gb, np.full((H, W), 8), cam, dict(gb=gb, cam=flat, history=hist))
    assert np.array_equal(out.view(np.uint32), inp.view(np.uint32)) and (h[..., 3] == 1.0).all()


def test_the_caps_hold():
    cam = _cam((0.0, 0.0, 0.0))
    gb = _gbuffer(cam, [(5.0, -1.0, 1.0, -1.0, 1.0), BACK])
    fill, _, _, _ = rr.writers(W, H, (W // 2, H // 2), 6, 16, 0)
    cfg = dict(history_fovea=2, history_middle=3, history_periphery=5)
    cap = tr.caps(fill, 0, cfg)
    assert {2, 3, 5} <= set(np.unique(cap).tolist()) <= {1, 2, 3, 5}
    prev = None
    for k in range(1, 8):
        out, h = tr.step(_frame(10 + k), gb, cap, cam, prev, cfg)
        assert (h[..., 3] <= cap).all()                         # exactly: n = fmin(n_h + 1, cap)
        # (a bilinear mean of equal lengths may round: n_h = (n w) / w)
        assert np.allclose(h[..., 3], np.minimum(k, cap), rtol=0, atol=1e-5)
        prev = dict(gb=gb, cam=cam, history=h)
    assert (tr.caps(fill, 1, dict(history_uniform=7))[fill > 0] == 7).all()


def test_cap_one_gives_the_input_bit_for_bit():
    cam = _cam((0.0, 0.0, 0.0))
    gb = _gbuffer(cam, [BACK])
    hist = np.concatenate([_frame(8)[..., :3], np.full((H, W, 1), 5.0, np.float32)], axis=-1)
    inp = _frame(9)
    inp[..., 3] = 0.25
    out, h = tr.step(inp, gb, np.ones((H, W), np.int64), cam, dict(gb=gb, cam=cam, history=hist))
    assert np.array_equal(out.view(np.uint32), inp.view(np.uint32)) and (h[..., 3] == 1.0).all()


def test_the_inverse_of_an_asymmetric_frustum():
    """setCameraFov's frusta: W is not orthogonal to U and V.  The fp32 inverse agrees with a float64 solve."""
    rng = np.random.default_rng(0)
    for _ in range(20):
        f = rng.normal(size=3)
        f /= np.linalg.norm(f)
        r_ = np.cross(f, (0.0, 1.0, 0.0))
        r_ /= np.linalg.norm(r_)
        u = np.cross(r_, f)
        tl, tr_, tu, td = np.tan(-rng.uniform(0.3, 0.9)), np.tan(rng.uniform(0.3, 0.9)), np.tan(rng.uniform(0.3, 0.9)), np.tan(-rng.uniform(0.3, 0.9))
        U = (0.5 * (tr_ - tl) * r_).astype(np.float32)
        V = (0.5 * (tu - td) * u).astype(np.float32)
        Wv = (f + 0.5 * (tr_ + tl) * r_ + 0.5 * (tu + td) * u).astype(np.float32)
        assert abs(float(np.dot(Wv, U))) > 1e-3 or abs(float(np.dot(Wv, V))) > 1e-3
        M = tr.camera_inverse(U, V, Wv)
        A = np.stack([U, V, Wv], axis=1).astype(np.float64)
        p = rng.normal(size=(100, 3))
        want = np.linalg.solve(A, p.T).T
        got = (p.astype(np.float32) @ M.T.astype(np.float64))
        assert np.allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
