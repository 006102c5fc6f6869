"""fovpt_warp_depth's restatement (tests/warp_depth_ref.py) without a GPU: with to == from every pixel that scatters lands on
itself, whatever its depth; pixels with NaN, zero, negative or -inf depth scatter nothing; on a G-buffer's own depths the
restatement agrees with fovpt_warp's (tests/warp_ref.py) where the rebuilt point rounds to the same pixel."""
import numpy as np
import pytest

import packet_depth_ref as pd
import warp_depth_ref as wd
import warp_ref as wr
from packet_depth_cases import camera_dict, synthetic_depth, synthetic_gbuffer

f32 = np.float32


def quantised(z, near):
    """Depths as a depth packet hands them back: the decoder's depth of the encoder's code."""
    return pd.depth_of_code(pd.code_of_depth(z, near), near)


@pytest.mark.parametrize("size", [(64, 48), (67, 49), (160, 96), (1920, 1080)], ids=lambda s: "%dx%d" % s)
def test_identity_every_pixel_lands_on_itself(size):
    """to == from: X = eye + z r, v = X - eye, and the projection of v is the pixel's own centre up to the roundings of these
    steps -- at most a few thousandths of a pixel, against the 0.5 that would move one.  All pixels, none excluded: raw depths
    over [0.01, 1e5], the same through a depth packet's code at near 0.05 and 0.1, and the sky."""
    w, h = size
    cam = camera_dict(size)
    rng = np.random.default_rng(w)
    raw = np.exp(rng.uniform(np.log(0.01), np.log(1e5), (h, w))).astype(np.float32)
    raw[rng.integers(0, 10, (h, w)) == 0] = np.inf
    own = np.arange(w * h, dtype=np.int64).reshape(h, w)
    Y, X = np.mgrid[0:h, 0:w]
    for label, depth in (("raw", raw), ("near 0.05", quantised(raw, 0.05)), ("near 0.1", quantised(raw, 0.1))):
        assert ((depth > 0) | np.isinf(depth)).all() and np.isinf(depth).any() and np.isfinite(depth).any()
        o = wd.warp(depth, cam, cam, dict(images=wr.RGBA, fill_radius=2), None, own.astype(np.uint32))
        assert np.array_equal(o["dest"], own), (label, int((o["dest"] != own).sum()))
        assert np.array_equal(o["map"], own.astype(np.uint32)) and o["counts"] == (w * h, w * h, 0, 0), label     # all class direct
        assert max(float(np.abs(o["px"] - X).max()), float(np.abs(o["py"] - Y).max())) < 0.05, label


def test_what_does_not_scatter_and_what_is_sky():
    size = (67, 49)
    w, h = size
    frm, to = camera_dict(size), camera_dict(size, (4.333, 3.0, 5.778), (0.333, 0.5, -0.222))
    depth = synthetic_depth(size, 4)
    dead = ~(depth > 0)
    assert np.isnan(depth).any() and (depth == 0).any() and (depth < 0).any() and np.isneginf(depth).any() and np.isposinf(depth).any()
    o = wd.warp(depth, frm, to, dict(images=wr.RGBA, fill_radius=0), None, np.arange(w * h, dtype=np.uint32).reshape(h, w))
    assert (o["dest"][dead] == -1).all() and (o["dest"][~dead] >= 0).sum() > w * h // 2
    sky = np.isposinf(depth)
    assert (o["depth"][sky] == wr.MISS_DEPTH).all() and (o["depth"][~sky & ~dead] != wr.MISS_DEPTH).all()
    srcs = o["map"][(o["map"] >> np.uint32(30)) == wr.DIRECT] & np.uint32(0x3fffffff)
    assert not dead.reshape(-1)[srcs].any()                                # no dead pixel is anybody's source
    assert o["counts"][0] == int((o["dest"] >= 0).sum()) and sum(o["counts"][1:]) == w * h
    # a translation does not move the sky; a pure rotation moves sky and surfaces alike
    far = np.full((h, w), np.inf, np.float32)
    o = wd.warp(far, frm, dict(to, U=frm["U"], V=frm["V"], W=frm["W"]), dict(images=wr.RGBA, fill_radius=0), None, np.zeros((h, w), np.uint32))
    assert np.array_equal(o["dest"], np.arange(w * h).reshape(h, w))


def test_on_a_gbuffers_own_depths_it_is_fovpt_warp():
    """depth = the G-buffer point's z along W (the quantity the packet codes, in binary64 here): the point rebuilt from it is the
    G-buffer's up to rounding, so the two warps send all but a few pixels near a rounding boundary to the same place, and the
    sky exactly."""
    size = (160, 96)
    w, h = size
    frm, to = camera_dict(size), camera_dict(size, (3.2, 2.5, 4.8))
    gb = synthetic_gbuffer(size, frm, 9, sky_blocks=False)
    M = wr.tr.camera_inverse(frm["U"], frm["V"], frm["W"]).astype(np.float64)
    v = gb["position"][..., :3].astype(np.float64) - np.asarray(frm["eye"], np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        z = (v @ M[2]).astype(np.float32)
    ok = np.isfinite(z) & (z > 0)
    miss = gb["prim"] == wr.MISS
    depth = np.where(miss, f32(np.inf), np.where(ok, z, f32(np.nan))).astype(np.float32)
    a, _ = wr.landing(gb, frm, to)
    b = wd.landing(depth, frm, to)[0]
    assert np.array_equal(a[miss], b[miss])
    sel = ok & ~miss
    assert sel.sum() > w * h // 2 and (a[sel] != b[sel]).mean() < 0.01
