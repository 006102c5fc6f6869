"""fovpt_gbuffer and fovpt_reconstruct on the GPU: the G-buffer bit for bit against the oracle's traversal and a numpy
restatement of the shading kernel's normal / albedo, the reconstruction bit for bit against tests/reconstruct_ref.py applied to
the GPU's own G-buffer and guides, inputs and later frames left untouched, error codes, ordering with frames in flight, the gain
in accuracy over the block-filled frame, and the C++ drop-in."""

import numpy as np
import pytest

import reconstruct_ref as rr
from fovpathtracing_optixcodelatest_amd import abi, lib, scenes

from common import cfg_foveated, cfg_uniform, make_gpu
from gpu_common import BOX_CAMERA, bits as _bits, box_model as _box_model, build_dropin, dropin_renderer, run_dropin
from postprocess_common import check_reconstruct as _check_bits, expected_gbuffer as _expected_gbuffer, rcfg as _rcfg

pytestmark = pytest.mark.gpu
E_INVALID, E_NO_SCENE, E_NO_FRAME = -1, -3, -5
# periphery RMSE against a 256-spp render, 384 x 216 atrium, radii 30 / 90, defaults (tools/reconstruct_perf.py --sweep,
# DESIGN.md 11): block-filled / reconstructed measured 2.12 on an MI355X, denoised / denoised + reconstructed 1.33; the tests
# keep a margin below the measured gains
QUALITY_MIN_GAIN = 1.8
QUALITY_MIN_GAIN_DENOISED = 1.2


def _atrium(size, cfg, gaze=None, tris=8000):
    cfg.write_guides = 1
    return make_gpu(scenes.atrium(tris), scenes.ambient_probe(96, 54, 2.5), scenes.ATRIUM_CAMERA, size, cfg, gaze=gaze)


@pytest.mark.parametrize("scene", ["cornell", "atrium", "sky", "odd"])
def test_gbuffer_matches_the_restatement(oracle, scene):
    cfg = cfg_foveated(10, 30)
    if scene == "cornell":
        model, cam, size, probe = scenes.cornell_box(), scenes.CORNELL_CAMERA, (96, 64), scenes.sky_probe()
    elif scene == "atrium":
        model, cam, size, probe = scenes.atrium(8000), scenes.ATRIUM_CAMERA, (160, 90), scenes.ambient_probe(96, 54, 2.5)
    else:
        model, cam, probe = _box_model(), BOX_CAMERA, scenes.ambient_probe(64, 32, 2.5)
        size = (128, 80) if scene == "sky" else (97, 61)
    r = make_gpu(model, probe, cam, size, cfg)
    got = r.downloadGBuffer()
    want = _expected_gbuffer(oracle, model, r)
    assert np.array_equal(got["prim"], want["prim"])
    for k in ("position", "normal", "albedo"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    miss = got["prim"] == rr.MISS
    if scene in ("sky", "odd"):
        assert 0.05 < miss.mean() < 0.95
    if scene == "atrium":
        textured = {k for k, m in enumerate(model.meshes) if m.texture_id >= 0 and m.texcoord is not None}
        assert textured and len(np.unique(got["albedo"][~miss][:, :3], axis=0)) > 100     # texels, not a few material colours
    # the production traversal: the same primitives as fovpt_debug_trace on the same rays
    f = r.launchParams.frame
    vec = lambda v: (v.x, v.y, v.z)
    o, d = rr.primary_rays(f.size.x, f.size.y, *(vec(getattr(r.launchParams.camera, n)) for n in ("eye", "U", "V", "W")))
    assert np.array_equal(r.debug_trace(o, d)[0].reshape(got["prim"].shape), got["prim"])
    r.close()


@pytest.mark.parametrize("gaze", ["centre", "corner"])
def test_reconstruct_matches_the_restatement_foveated(oracle, gaze):
    cfg = cfg_foveated(15, 48, (1, 2, 8))
    r = _atrium((193, 109), cfg, gaze=(96, 54) if gaze == "centre" else (3, 105))
    r.render()
    out, fill = _check_bits(oracle, r, cfg)
    acc = r.downloadAccum()
    assert {1, 2, 4} <= set(np.unique(fill).tolist())
    assert not np.array_equal(out[fill == 4], acc[fill == 4])                    # (it did reconstruct)
    for d in (dict(levels=1), dict(levels=2), dict(levels=0), dict(remodulate=0),
              dict(support=2.0, normal_sigma=0.2, depth_sigma=0.5), dict(support=1.5, depth_sigma=0.01, remodulate=0)):
        _check_bits(oracle, r, cfg, d)
    r.close()


def test_reconstruct_is_the_identity_on_uniform_frames(oracle):
    cfg = cfg_uniform(1)
    r = _atrium((160, 90), cfg)
    r.render()
    out, fill = _check_bits(oracle, r, cfg)
    assert (fill == 1).all()
    assert np.array_equal(_bits(out), _bits(r.downloadAccum()))
    assert np.array_equal(r.downloadReconstructedPixels(), r.downloadPixels())
    r.close()


def test_reconstruct_matches_the_restatement_accumulating(oracle):
    cfg = cfg_foveated(15, 48, (1, 2, 8))
    cfg.accumulate = 1
    r = _atrium((192, 108), cfg)
    r.render()
    r.render()
    _check_bits(oracle, r, cfg)
    r.close()


def test_reconstruct_of_the_denoised_frame(oracle):
    cfg = cfg_foveated(15, 48, (1, 2, 8))
    r = _atrium((192, 108), cfg)
    r.render()
    r.denoise()
    den_ptr = r.denoise_buffers()[0]
    _check_bits(oracle, r, cfg, in_color=r.downloadDenoisedColor(), in_ptr=den_ptr)
    r.close()


def test_reconstruct_leaves_its_inputs_and_the_next_frames_alone():
    cfg = cfg_foveated(15, 48, (1, 2, 8))
    frames = []
    for with_calls in (False, True):
        r = _atrium((192, 108), cfg)
        f = r.launchParams.frame
        shape = (f.size.y, f.size.x, 4)
        seq = []
        for k in range(3):
            f.c.x, f.c.y = 60 + 30 * k, 50 + 5 * k
            r.render()
            bufs = [r.downloadAccum(), r.downloadPixels()] + [r.download(p, np.empty(shape, np.float32))
                                                              for p in (f.color_buffer, f.normal_buffer, f.albedo_buffer)]
            if with_calls:
                r.gbuffer()
                r.reconstruct()
                fill, _, _, _ = rr.writers(f.size.x, f.size.y, (f.c.x, f.c.y), cfg.r_inner, cfg.r_outer, 0)
                px = r.downloadReconstructedPixels()
                assert np.array_equal(px[fill == 1], bufs[1][fill == 1])            # fill-1 pixels: the resolve's rgba8
                after = [r.downloadAccum(), r.downloadPixels()] + [r.download(p, np.empty(shape, np.float32))
                                                                   for p in (f.color_buffer, f.normal_buffer, f.albedo_buffer)]
                for a, b in zip(bufs, after):
                    assert np.array_equal(_bits(a), _bits(b))
            seq.append(bufs)
        s = r.stats()
        seq.append([s.radiance_rays, s.shadow_rays, s.paths, s.frames])
        frames.append(seq)
        r.close()
    for a, b in zip(frames[0][:-1], frames[1][:-1]):
        for x, y in zip(a, b):
            assert np.array_equal(_bits(x), _bits(y))
    assert frames[0][-1] == frames[1][-1]


def test_reconstruct_errors():
    cfg = cfg_foveated(15, 48, (1, 2, 8))
    r = _atrium((96, 64), cfg)
    with pytest.raises(lib.FovptError) as e:             # nothing rendered yet
        r.reconstruct()
    assert e.value.code == E_NO_FRAME
    r.render()
    r.reconstruct()
    outside = (float(np.nextafter(np.float32(abi.SIGMA_MIN), np.float32(0))), float(np.nextafter(np.float32(abi.SIGMA_MAX), np.float32(np.inf))))
    for k, v in (("support", 0.5), ("support", 2.5), ("support", float("nan")), ("normal_sigma", 0.0), ("depth_sigma", float("inf")),
                 ("depth_sigma", -1.0), ("levels", 4), ("levels", -1), ("remodulate", 2)) + tuple(
                     (k, v) for k in ("normal_sigma", "depth_sigma") for v in outside):
        with pytest.raises(lib.FovptError) as e:
            r.reconstruct(_rcfg({k: v}))
        assert e.value.code == E_INVALID, (k, v)
    r.reconstruct(_rcfg(dict(normal_sigma=abi.SIGMA_MIN, depth_sigma=abi.SIGMA_MAX)))  # the bounds themselves are accepted
    r.reconstruct(_rcfg(dict(normal_sigma=abi.SIGMA_MAX, depth_sigma=abi.SIGMA_MIN)))
    bad = _rcfg(None)
    bad._reserved[1] = 1
    with pytest.raises(lib.FovptError) as e:
        r.reconstruct(bad)
    assert e.value.code == E_INVALID
    col, _ = r.reconstruct_buffers()
    with pytest.raises(lib.FovptError) as e:             # reading the buffer it writes
        r.reconstruct(None, col, None, None)
    assert e.value.code == E_INVALID
    with pytest.raises(lib.FovptError) as e:
        r.reconstruct(None, None, r.launchParams.frame.accum_buffer, None)
    assert e.value.code == E_INVALID
    f = r.launchParams.frame
    f.size.x -= 4
    with pytest.raises(lib.FovptError) as e:
        r.reconstruct()
    assert e.value.code == E_NO_FRAME
    f.size.x += 4
    trav = r.launchParams.traversable
    r.launchParams.traversable = 12345
    for call in (r.reconstruct, r.gbuffer):
        with pytest.raises(lib.FovptError) as e:
            call()
        assert e.value.code == E_NO_SCENE
    r.launchParams.traversable = trav
    L = lib.load()
    assert L.fovpt_reconstruct(r._ctx, None, None, None, None, None) == E_INVALID
    assert L.fovpt_gbuffer(r._ctx, None, None) == E_INVALID
    c = r.config
    c.write_guides = 0
    r.config = c
    r.render()
    with pytest.raises(lib.FovptError) as e:
        r.reconstruct()
    assert e.value.code == E_INVALID and "write_guides" in str(e.value)
    r.reconstruct(_rcfg(dict(remodulate=0)))             # without remodulation it needs no guides
    c.write_guides, c.world, c.rank = 1, 2, 0
    r.config = c
    r.render()
    with pytest.raises(lib.FovptError) as e:
        r.reconstruct()
    assert e.value.code == E_INVALID
    r.close()


@pytest.mark.parametrize("mode", ["frames_in_flight", "chains_per_frame"])
def test_reconstruct_is_ordered_with_frames_in_flight(mode):
    """Four frames with a moving gaze and camera, issued back to back with a reconstruct after each into caller buffers, give
    what the same frames rendered one at a time with a synchronise after each give."""
    import torch
    size = (384, 216)
    cfg = cfg_foveated(20, 60, (4, 8, 16))               # >= 16384 sample slots: chains_per_frame = 2 does split the frame
    if mode == "frames_in_flight":
        cfg.frames_in_flight = 2
    else:
        cfg.chains_per_frame = 2
    r = _atrium(size, cfg)
    from fovpathtracing_optixcodelatest_amd import renderer
    cam = scenes.ATRIUM_CAMERA
    views = [((120 + 40 * k, 90 + 15 * k), (cam["eye"][0] + 40.0 * k, cam["eye"][1], cam["eye"][2] + 25.0 * k)) for k in range(4)]

    def setup(g, eye):
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = g
        r.launchParams.frame.subframe_index = 0
        r.setCamera(renderer.Camera(eye, cam["lookat"], cam["up"], cam["fovy"], size[0] / float(size[1])))

    # the pixels no pass writes keep the previous frame's values: the synchronous frames get the same history (last, then all)
    want = []
    for g, eye in views[-1:] + views:
        setup(g, eye)
        r.render()
        r.synchronize()
        r.reconstruct()
        want.append((r.downloadReconstructedColor(), r.downloadReconstructedPixels()))
    want = want[1:]
    outs = [(torch.empty((size[1], size[0], 4), dtype=torch.float32, device="cuda"),
             torch.empty((size[1], size[0]), dtype=torch.int32, device="cuda")) for _ in views]
    torch.cuda.synchronize()
    for (g, eye), (oc, op) in zip(views, outs):
        setup(g, eye)
        r.render_async()
        r.reconstruct(None, None, oc.data_ptr(), op.data_ptr())
    r.synchronize()
    for (wc, wp), (oc, op) in zip(want, outs):
        assert np.array_equal(_bits(oc.cpu().numpy()), _bits(wc))
        assert np.array_equal(op.cpu().numpy().view(np.uint32), wp)
    assert not np.array_equal(want[0][1], want[1][1])
    r.close()


def _rmse(img, truth, mask):
    d = img[..., :3].astype(np.float64) - truth[..., :3]
    return float(np.sqrt((d[mask] ** 2).mean()))


def test_reconstruct_reduces_the_periphery_error():
    """The truth is the GPU's own FOV_OFF render at 256 spp of the same view.  Periphery RMSE: block-filled vs reconstructed,
    and denoised vs denoised + reconstructed."""
    size = (384, 216)
    t = _atrium(size, cfg_uniform(256))
    t.render()
    truth = t.downloadAccum()
    t.close()
    cfg = cfg_foveated(30, 90, (1, 2, 8))
    r = _atrium(size, cfg)
    r.render()
    raw = r.downloadAccum()
    r.reconstruct()
    rec = r.downloadReconstructedColor()
    r.denoise()
    den = r.downloadDenoisedColor()
    r.reconstruct(None, r.denoise_buffers()[0])
    den_rec = r.downloadReconstructedColor()
    f = r.launchParams.frame
    fill, _, _, _ = rr.writers(size[0], size[1], (f.c.x, f.c.y), cfg.r_inner, cfg.r_outer, 0)
    per = fill == 4
    gain = _rmse(raw, truth, per) / _rmse(rec, truth, per)
    gain_den = _rmse(den, truth, per) / _rmse(den_rec, truth, per)
    print("periphery RMSE gain: reconstructed %.3f, denoised + reconstructed %.3f" % (gain, gain_den))
    assert gain >= QUALITY_MIN_GAIN
    assert gain_den >= QUALITY_MIN_GAIN_DENOISED
    r.close()


def test_cpp_dropin_reconstruct(tmp_path):
    """SampleRenderer::reconstruct() + downloadReconstructedPixels of include/SimplePathtracer.h: the same pixels as Python."""
    exe, out = build_dropin(tmp_path, "reconstruct_gpu_test"), str(tmp_path / "reconstruct_out.bin")
    run_dropin(exe, out)
    px = np.fromfile(out, np.uint32).reshape(2, 96, 160)
    r = dropin_renderer(write_guides=True)
    r.render()
    r.reconstruct()
    assert np.array_equal(px[0], r.downloadPixels())
    assert np.array_equal(px[1], r.downloadReconstructedPixels())
    assert not np.array_equal(px[0], px[1])
    r.close()
