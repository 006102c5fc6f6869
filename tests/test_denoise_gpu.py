"""fovpt_denoise on the GPU: bit for bit the numpy restatement (tests/denoise_ref.py) applied to the GPU's own guide buffers,
inputs left untouched, error codes, ordering with frames in flight, the gain in accuracy over the raw foveated frame, and the
C++ drop-in."""

import numpy as np
import pytest

import denoise_ref as dn
from fovpathtracing_optixcodelatest_amd import abi, lib, scenes

from common import cfg_foveated, cfg_uniform, make_gpu
from gpu_common import bits as _bits, build_dropin, dropin_renderer, run_dropin
from postprocess_common import check_denoise as _check_bits, dcfg as _dcfg, guides as _guides

pytestmark = pytest.mark.gpu
E_INVALID, E_NO_FRAME = -1, -5
SIGMAS = ("color_sigma", "normal_sigma", "albedo_sigma")
# the binary32 neighbours just outside [FOVPT_SIGMA_MIN, FOVPT_SIGMA_MAX]
SIGMA_OUTSIDE = (float(np.nextafter(np.float32(abi.SIGMA_MIN), np.float32(0))), float(np.nextafter(np.float32(abi.SIGMA_MAX), np.float32(np.inf))))
# periphery RMSE (raw foveated frame) / periphery RMSE (denoised, defaults) against a 256-spp render, 384 x 216 atrium:
# measured 2.27 on an MI355X (middle ring 2.28; tools/denoise_perf.py --sweep); the test keeps a margin below that
QUALITY_MIN_GAIN = 1.8


def _atrium(size, cfg, gaze=None, tris=8000):
    cfg.write_guides = 1
    return make_gpu(scenes.atrium(tris), scenes.ambient_probe(96, 54, 2.5), scenes.ATRIUM_CAMERA, size, cfg, gaze=gaze)


@pytest.mark.parametrize("gaze", ["centre", "corner"])
def test_denoise_matches_the_restatement_foveated(oracle, gaze):
    size = (192, 108)
    cfg = cfg_foveated(15, 48, (1, 2, 8))
    r = _atrium(size, cfg, gaze=(96, 54) if gaze == "centre" else (10, 100))
    r.render()
    _, n, pas = _check_bits(oracle, r, cfg)
    assert n.max() == 3 and {0, 1, 2} <= set(np.unique(pas).tolist())
    _check_bits(oracle, r, cfg, dict(iterations_fovea=1, iterations_middle=4, iterations_periphery=5, color_sigma=2.0,
                                     normal_sigma=0.3, albedo_sigma=0.25))
    r.close()


def test_denoise_matches_the_restatement_uniform(oracle):
    cfg = cfg_uniform(1)
    r = _atrium((192, 108), cfg)
    r.render()
    _, n, _ = _check_bits(oracle, r, cfg)
    assert (n == 3).all()
    r.close()


def test_denoise_matches_the_restatement_accumulating(oracle):
    cfg = cfg_foveated(15, 48, (1, 2, 8))
    cfg.accumulate = 1
    r = _atrium((192, 108), cfg)
    r.render()
    r.render()                                   # subframe 1: the resolve blends with the first
    assert r.launchParams.frame.subframe_index == 2
    _check_bits(oracle, r, cfg)
    r.close()


def test_denoise_matches_the_restatement_c3(oracle):
    """BASELINE C3: 262,144-triangle atrium at 1920 x 1080, radii 148 / 482, spp 1 / 2 / 8, defaults."""
    cfg = cfg_foveated(148, 482, (1, 2, 8))
    r = _atrium((1920, 1080), cfg, tris=262144)
    r.render()
    _check_bits(oracle, r, cfg)
    r.close()


def test_denoise_leaves_its_inputs_and_the_fovea_alone():
    cfg = cfg_foveated(15, 48, (1, 2, 8))
    r = _atrium((192, 108), cfg)
    r.render()
    f = r.launchParams.frame
    before = _guides(r) + [r.downloadAccum(), r.downloadPixels()]
    r.denoise()
    out_c, out_px = r.downloadDenoisedColor(), r.downloadDenoisedPixels()
    after = _guides(r) + [r.downloadAccum(), r.downloadPixels()]
    for a, b in zip(before, after):
        assert np.array_equal(_bits(a), _bits(b))
    fill, pas = dn.level_map(f.size.x, f.size.y, (f.c.x, f.c.y), cfg.r_inner, cfg.r_outer, 0)
    fovea = pas == 2
    assert fovea.sum() > 500
    accum, frame = before[3], before[4]
    assert np.array_equal(_bits(out_c[fovea]), _bits(accum[fovea]))
    assert np.array_equal(out_px[fovea], frame[fovea])
    assert not np.array_equal(out_c[pas == 0], accum[pas == 0])          # (the periphery is filtered)
    r.close()


def test_denoise_errors():
    cfg = cfg_foveated(15, 48, (1, 2, 8))
    r = _atrium((96, 64), cfg)
    with pytest.raises(lib.FovptError) as e:             # nothing rendered yet
        r.denoise()
    assert e.value.code == E_NO_FRAME
    r.render()
    r.denoise()
    for k, v in (("iterations_middle", 6), ("iterations_fovea", -1), ("color_sigma", 0.0), ("normal_sigma", float("inf")),
                 ("albedo_sigma", float("nan"))) + tuple((k, v) for k in SIGMAS for v in SIGMA_OUTSIDE):
        with pytest.raises(lib.FovptError) as e:
            r.denoise(_dcfg({k: v}))
        assert e.value.code == E_INVALID, (k, v)
    r.denoise(_dcfg({k: abi.SIGMA_MIN for k in SIGMAS}))  # the bounds themselves are accepted
    r.denoise(_dcfg({k: abi.SIGMA_MAX for k in SIGMAS}))
    f = r.launchParams.frame
    f.size.x -= 4                                        # not the size of the frame last rendered
    with pytest.raises(lib.FovptError) as e:
        r.denoise()
    assert e.value.code == E_NO_FRAME
    f.size.x += 4
    c = r.config
    c.write_guides = 0
    r.config = c
    r.render()
    with pytest.raises(lib.FovptError) as e:
        r.denoise()
    assert e.value.code == E_INVALID and "write_guides" in str(e.value)
    c.write_guides, c.world, c.rank = 1, 2, 0
    r.config = c
    r.render()
    with pytest.raises(lib.FovptError) as e:
        r.denoise()
    assert e.value.code == E_INVALID
    r.close()


@pytest.mark.parametrize("mode", ["frames_in_flight", "chains_per_frame"])
def test_denoise_is_ordered_with_frames_in_flight(mode):
    """render_async (gaze A) -> denoise(out = X) -> render_async (gaze B) -> denoise(out = Y) -> sync gives, per frame, what
    render + sync + denoise gives."""
    import torch
    size = (384, 216)
    cfg = cfg_foveated(20, 60, (4, 8, 16))               # >= 16384 sample slots: chains_per_frame = 2 does split the frame
    if mode == "frames_in_flight":
        cfg.frames_in_flight = 2
    else:
        cfg.chains_per_frame = 2
    r = _atrium(size, cfg)
    gazes = [(120, 90), (250, 140)]
    want = []
    # the pixels no pass writes (between the rings) keep the previous frame's values, as in the reference: the synchronous
    # frames are rendered with the same history as the asynchronous ones (B, then A, B)
    for g in gazes[1:] + gazes:
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = g
        r.launchParams.frame.subframe_index = 0
        r.render()
        r.denoise()
        want.append((r.downloadDenoisedColor(), r.downloadDenoisedPixels()))
    want = want[1:]
    outs = [(torch.empty((size[1], size[0], 4), dtype=torch.float32, device="cuda"),
             torch.empty((size[1], size[0]), dtype=torch.int32, device="cuda")) for _ in gazes]
    torch.cuda.synchronize()
    for g, (oc, op) in zip(gazes, outs):
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = g
        r.launchParams.frame.subframe_index = 0
        r.render_async()
        r.denoise(None, oc.data_ptr(), op.data_ptr())
    r.synchronize()
    for (wc, wp), (oc, op) in zip(want, outs):
        assert np.array_equal(_bits(oc.cpu().numpy()), _bits(wc))
        assert np.array_equal(op.cpu().numpy().view(np.uint32), wp)
    assert not np.array_equal(want[0][1], want[1][1])
    r.close()


def _periphery_rmse(img, truth, mask):
    d = img[..., :3].astype(np.float64) - truth[..., :3]
    return float(np.sqrt((d[mask] ** 2).mean()))


def test_denoise_reduces_the_periphery_error():
    """Same scene and camera; the truth is the GPU's own FOV_OFF render at 256 spp.  The periphery's error (1 sample per 4 x 4
    block) drops by at least QUALITY_MIN_GAIN under the default configuration."""
    size = (384, 216)
    t = _atrium(size, cfg_uniform(256))
    t.render()
    truth = t.downloadAccum()
    t.close()
    cfg = cfg_foveated(30, 90, (1, 2, 8))
    r = _atrium(size, cfg)
    r.render()
    raw = r.downloadAccum()
    r.denoise()
    den = r.downloadDenoisedColor()
    f = r.launchParams.frame
    _, pas = dn.level_map(size[0], size[1], (f.c.x, f.c.y), cfg.r_inner, cfg.r_outer, 0)
    per, mid = pas == 0, pas == 1
    gain = _periphery_rmse(raw, truth, per) / _periphery_rmse(den, truth, per)
    gain_mid = _periphery_rmse(raw, truth, mid) / _periphery_rmse(den, truth, mid)
    print("periphery RMSE gain %.3f, middle ring %.3f" % (gain, gain_mid))
    assert gain >= QUALITY_MIN_GAIN
    assert gain_mid >= 1.5
    r.close()


def test_cpp_dropin_denoise(tmp_path):
    """SampleRenderer::denoise() + downloadDenoisedPixels of include/SimplePathtracer.h: the same pixels as the Python surface."""
    exe, out = build_dropin(tmp_path, "denoise_gpu_test"), str(tmp_path / "denoise_out.bin")
    run_dropin(exe, out)
    px = np.fromfile(out, np.uint32).reshape(2, 96, 160)
    r = dropin_renderer(write_guides=True)
    r.render()
    r.denoise()
    assert np.array_equal(px[0], r.downloadPixels())
    assert np.array_equal(px[1], r.downloadDenoisedPixels())
    assert not np.array_equal(px[0], px[1])
    r.close()
