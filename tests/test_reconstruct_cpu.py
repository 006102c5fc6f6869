"""fovpt_reconstruct without a GPU: the C ABI of its structs (layout, defaults, argument checks) and properties of the
reconstruction's definition, the numpy restatement in tests/reconstruct_ref.py that the GPU kernels are checked against."""
import ctypes as C

import numpy as np
import pytest

import header_layout
import reconstruct_ref as rr
from fovpathtracing_optixcodelatest_amd import abi, lib


@pytest.fixture(scope="module")
def so():
    lib.build()
    return lib.load()


@pytest.mark.parametrize("struct, cname, size", [(abi.ReconstructConfig, "fovpt_reconstruct_config", 32),
                                                 (abi.GBufferPtrs, "fovpt_gbuffer_ptrs", 40)])
def test_struct_mirrors_match_the_header(struct, cname, size):
    names = [f[0] for f in struct._fields_]
    got = header_layout.layout(cname, struct)
    assert got[0] == C.sizeof(struct) == size
    assert got[1:] == [getattr(struct, n).offset for n in names]


def test_reconstruct_defaults_are_documented_and_in_range(so):
    d = abi.ReconstructConfig()
    assert so.fovpt_reconstruct_defaults(C.byref(d)) == 0
    assert d.as_dict() == {k: np.float32(v) if isinstance(v, float) else v for k, v in rr.DEFAULTS.items()}
    assert 1.0 <= d.support <= 2.0 and 0 < d.normal_sigma < np.inf and 0 < d.depth_sigma < np.inf
    assert d.levels in range(4) and d.remodulate in (0, 1) and list(d._reserved) == [0, 0, 0]
    assert so.fovpt_reconstruct_defaults(None) == -1


def test_reconstruct_rejects_null_arguments(so):
    d = abi.ReconstructConfig()
    so.fovpt_reconstruct_defaults(C.byref(d))
    lp = abi.LaunchParams()
    assert so.fovpt_reconstruct(None, C.byref(lp), C.byref(d), None, None, None) == -1
    assert so.fovpt_gbuffer(None, C.byref(lp), None) == -1
    col, rgba = C.c_void_p(), C.c_void_p()
    assert so.fovpt_reconstruct_buffers(None, C.byref(col), C.byref(rgba)) == -1


W, H, GAZE, RI, RO = 64, 48, (32, 24), 6, 16


def _flat_gbuffer(albedo=None):
    """A plane z = 10 seen head on: every pixel a hit, normal (0, 0, -1)."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    pos = np.zeros((H, W, 4), np.float32)
    pos[..., 0], pos[..., 1], pos[..., 2], pos[..., 3] = x * np.float32(0.1), y * np.float32(0.1), 10.0, 10.0
    nrm = np.zeros((H, W, 4), np.float32)
    nrm[..., 2] = -1.0
    alb = np.zeros((H, W, 4), np.float32)
    alb[..., :3] = 0.5 if albedo is None else albedo
    return dict(prim=np.zeros((H, W), np.uint32), position=pos, normal=nrm, albedo=alb)


def _writers():
    fill, pas, ax, ay = rr.writers(W, H, GAZE, RI, RO, 0)
    assert {1, 2, 4} <= set(np.unique(fill).tolist())
    return fill, pas, ax, ay


def _block_copy(img, fill, ax, ay):
    """What the resolve's block fill does: every written pixel holds the value at its anchor."""
    out = img.copy()
    m = fill > 0
    out[m] = img[np.minimum(ay[m], H - 1), np.minimum(ax[m], W - 1)]
    return out


def test_writers_agree_with_the_denoisers_level_map():
    import denoise_ref as dn
    for gaze, uni in (((32, 24), 0), ((2, 45), 0), ((200, 200), 0), ((10, 10), 1)):
        fill, pas, ax, ay = rr.writers(W, H, gaze, RI, RO, uni)
        f2, p2 = dn.level_map(W, H, gaze, RI, RO, uni)
        assert np.array_equal(fill, f2) and np.array_equal(pas, p2)
        m = (fill > 0) & (ax < W) & (ay < H)                # (anchors beyond the frame are clamped onto its last row / column)
        xs, ys = np.meshgrid(np.arange(W), np.arange(H))
        assert (ax[m] <= xs[m]).all() and (xs[m] < ax[m] + fill[m]).all() and (ay[m] <= ys[m]).all() and (ys[m] < ay[m] + fill[m]).all()


def test_a_constant_image_stays_constant():
    fill, _, ax, ay = _writers()
    img = np.full((H, W, 4), 0.75, np.float32)
    img[..., 3] = 1
    gb = _flat_gbuffer()
    for remod in (0, 1):
        out = rr.reconstruct(img, gb["albedo"], gb, fill, ax, ay, dict(remodulate=remod))
        np.testing.assert_allclose(out[..., :3], 0.75, rtol=1e-6)
        assert (out[..., 3] == 1).all()


def test_fovea_and_masked_levels_are_untouched():
    fill, _, ax, ay = _writers()
    rng = np.random.default_rng(1)
    img = rng.uniform(0, 2, (H, W, 4)).astype(np.float32)
    gb = _flat_gbuffer()
    for levels in range(4):
        out = rr.reconstruct(img, gb["albedo"], gb, fill, ax, ay, dict(levels=levels))
        keep = (fill <= 1) | ((fill == 2) & (levels & 1 == 0)) | ((fill == 4) & (levels & 2 == 0))
        assert np.array_equal(out[keep].view(np.uint32), img[keep].view(np.uint32))
        assert (out[~keep][:, 3] == 1).all()
        assert not np.array_equal(out[~keep], img[~keep]) or (~keep).sum() == 0
    fill_u, _, axu, ayu = rr.writers(W, H, GAZE, RI, RO, 1)
    assert np.array_equal(rr.reconstruct(img, gb["albedo"], gb, fill_u, axu, ayu).view(np.uint32), img.view(np.uint32))


def test_no_weight_leaves_the_pixel_unchanged():
    """A hit pixel whose candidates are all misses (and a miss whose candidates are all hits) has sum w = 0."""
    fill, _, ax, ay = _writers()
    img = np.random.default_rng(2).uniform(0, 2, (H, W, 4)).astype(np.float32)
    gb = _flat_gbuffer()
    gb["prim"][:] = rr.MISS
    p = (2, 3)                                            # a periphery pixel that is not an anchor
    assert fill[p] == 4 and (ax[p], ay[p]) != (p[1], p[0])
    gb["prim"][p] = 0
    out = rr.reconstruct(img, gb["albedo"], gb, fill, ax, ay)
    assert np.array_equal(out[p].view(np.uint32), img[p].view(np.uint32))
    gb2 = _flat_gbuffer()
    gb2["prim"][p] = rr.MISS
    out = rr.reconstruct(img, gb2["albedo"], gb2, fill, ax, ay)
    assert np.array_equal(out[p].view(np.uint32), img[p].view(np.uint32))


def test_remodulation_recovers_the_texture_a_block_copy_loses():
    """Flat geometry under constant illumination 1: the rendered colour and albedo guide are block copies of the texture at the
    anchors, the G-buffer has the texture at every pixel.  remodulate = 1 gives back the texture exactly; the block copy (and
    remodulate = 0) does not."""
    fill, _, ax, ay = _writers()
    y, x = np.mgrid[0:H, 0:W]
    tex = np.where(((x + y) % 2 == 0)[..., None], np.float32([0.8, 0.3, 0.2]), np.float32([0.1, 0.6, 0.9])).astype(np.float32)
    tex4 = np.concatenate([tex, np.ones((H, W, 1), np.float32)], axis=-1)
    guide = _block_copy(tex4, fill, ax, ay)
    color = guide.copy()                                  # radiance = illumination 1 x albedo of the sample
    gb = _flat_gbuffer(tex)
    out = rr.reconstruct(color, guide, gb, fill, ax, ay)
    rec = fill > 1
    assert np.array_equal(out[rec][:, :3], tex[rec])
    assert not np.array_equal(color[rec][:, :3], tex[rec])
    out0 = rr.reconstruct(color, guide, gb, fill, ax, ay, dict(remodulate=0))
    assert not np.array_equal(out0[rec][:, :3], tex[rec])


def test_depth_and_normal_edges_stop_the_weights():
    """Two planes at different depths (or facing different ways) left and right of x = 30: no pixel takes colour across."""
    fill, _, ax, ay = _writers()
    img = np.zeros((H, W, 4), np.float32)
    img[:, :30, :3], img[:, 30:, :3] = 1.0, 5.0
    img[..., 3] = 1
    for edge in ("depth", "normal"):
        gb = _flat_gbuffer()
        if edge == "depth":
            gb["position"][:, 30:, 2] = 20.0
            gb["position"][:, 30:, 3] = 20.0
        else:
            gb["normal"][:, 30:, :3] = np.float32([1.0, 0.0, 0.0])
        out = rr.reconstruct(img, gb["albedo"], gb, fill, ax, ay, dict(remodulate=0))
        left, right = np.arange(W) < 30, np.arange(W) >= 30
        assert (out[:, left, :3] == 1.0).all() or np.allclose(out[:, left, :3], 1.0, rtol=1e-6)
        assert np.allclose(out[:, right, :3], 5.0, rtol=1e-6)


def test_primary_rays_are_the_centre_of_each_pixel():
    o, d = rr.primary_rays(4, 2, (1, 2, 3), (1, 0, 0), (0, 1, 0), (0, 0, -2))
    assert o.shape == d.shape == (8, 3) and (o == np.float32([1, 2, 3])).all()
    np.testing.assert_allclose(np.linalg.norm(d, axis=1), 1.0, rtol=1e-6)
    assert d[0, 0] < 0 and d[0, 1] < 0 and d[7, 0] > 0 and d[7, 1] > 0
    np.testing.assert_allclose(d[:, 0], -d[::-1, 0], rtol=1e-6)
