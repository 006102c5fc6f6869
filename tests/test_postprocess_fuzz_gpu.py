"""Post-processing of rendered frames on the GPU beyond the hand-picked frames of test_denoise_gpu.py / test_reconstruct_gpu.py:
a seeded fuzz of fovpt_denoise, fovpt_gbuffer and fovpt_reconstruct over frame sizes (from 1 x 1), gazes off the frame, radii,
FOV_OFF, accumulation, scenes and configs (tests/postprocess_fuzz.py draws them), bit for bit against the numpy restatements
and the oracle; reconstruction at the full C3 and C5 (one eye) sizes; and post-processing of the frame as it was rendered
when the caller has moved on to the next gaze, config, camera or frame size."""
import numpy as np
import pytest

import postprocess_fuzz as pf
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer, scenes

from common import cfg_foveated, cfg_uniform, make_gpu, make_oracle
from gpu_common import bits, BOX_CAMERA, box_model
from postprocess_common import check_denoise, check_gbuffer_prim, check_reconstruct, expected_gbuffer, expected_reconstruct, rcfg

pytestmark = pytest.mark.gpu
E_INVALID, E_NO_FRAME = -1, -5
GBUFFER_FULL_MAX = 20000          # frames up to this many pixels: all four G-buffer planes against the oracle restatement
SOUP_CAMERA = dict(eye=(0.0, 2.5, 11.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fovy=50.0)


def _soup(seed):
    """A few random triangle meshes, the first one textured (texture of any size, texcoords that wrap)."""
    rng = np.random.default_rng(seed)
    meshes, textures = [], []
    for m in range(int(rng.integers(1, 4))):
        n = int(rng.integers(1, 80))
        centre = rng.uniform(-4, 4, (n, 1, 3)) * np.float32([1.0, 0.4, 1.0])
        v = (centre + rng.uniform(-1.2, 1.2, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
        mat = abi.Material.reference_default()
        mat.color.set(rng.uniform(0, 1, 3))
        mat.emission.set(rng.uniform(0, 3, 3) if rng.random() < 0.3 else (0, 0, 0))
        tc, tid = None, -1
        if m == 0:
            textures.append(rng.integers(0, 2 ** 32, (int(rng.integers(1, 9)), int(rng.integers(1, 9))), dtype=np.uint64).astype(np.uint32))
            tid = 0
            tc = rng.uniform(-2, 3, (3 * n, 2)).astype(np.float32)
        meshes.append(scenes.TriangleMesh(vertex=v, index=np.arange(3 * n, dtype=np.uint32).reshape(n, 3), material=mat,
                                          texcoord=tc, texture_id=tid))
    return scenes.Model(meshes=meshes, textures=textures)


def _scene(p):
    if p["scene"] == "atrium":
        tris = int(np.random.default_rng(p["scene_seed"]).integers(1000, 6000))
        return scenes.atrium(tris, seed=p["scene_seed"]), scenes.ATRIUM_CAMERA, scenes.ambient_probe(96, 54, 2.5)
    if p["scene"] == "box":
        return box_model(), BOX_CAMERA, scenes.sky_probe()
    return _soup(p["scene_seed"]), SOUP_CAMERA, scenes.ambient_probe(32, 16, 1.0)


def _config(p):
    spp_p, spp_m, spp_f, spp_u = p["spp"]
    if p["uniform"]:
        cfg = cfg_uniform(spp_u, max_depth=p["max_depth"])
    else:
        cfg = cfg_foveated(p["radii"][0], p["radii"][1], (spp_p, spp_m, spp_f), max_depth=p["max_depth"])
    cfg.r_inner, cfg.r_outer = p["radii"]                # (FOV_OFF frames ignore them)
    cfg.accumulate, cfg.write_guides = p["accumulate"], p["write_guides"]
    return cfg


@pytest.mark.parametrize("seed", pf.SEEDS)
def test_random_postprocessing(oracle, seed):
    """One seeded frame (tests/postprocess_fuzz.py): denoise, G-buffer and reconstruction bit for bit against their
    restatements over the GPU's own inputs; frames smaller than the main-path fuzz renders also against the oracle."""
    import torch
    p = pf.params(seed)
    model, cam, probe = _scene(p)
    (w, h), gaze = p["size"], p["gaze"]
    cfg = _config(p)
    r = make_gpu(model, probe, cam, (w, h), cfg, gaze=gaze)
    frames = 2 if p["accumulate"] else 1
    for _ in range(frames):
        r.render()
    if w < 17 or h < 9:
        S, F = make_oracle(oracle, model, probe, cam, (w, h), gaze=gaze)
        for _ in range(frames):
            oracle.render(S, F, cfg)
        assert np.array_equal(bits(r.downloadAccum()), bits(F.accum)) and np.array_equal(r.downloadPixels(), F.frame), p

    in_color, in_ptr = None, None
    if p["denoise"] is None:                             # rendered without guides: nothing to filter with
        with pytest.raises(lib.FovptError) as e:
            r.denoise()
        assert e.value.code == E_INVALID
    else:
        check_denoise(oracle, r, cfg, p["denoise"])
        if p["reconstruct_input"] == "denoised":
            in_color, in_ptr = r.downloadDenoisedColor(), r.denoise_buffers()[0]

    rc = p["reconstruct"]
    if p["caller_buffers"]:
        oc = torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda")
        op = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.reconstruct(rcfg(rc), in_ptr, oc.data_ptr(), op.data_ptr())
        r.synchronize()
        got_c, got_px = oc.cpu().numpy(), op.cpu().numpy().view(np.uint32)
    else:
        r.reconstruct(rcfg(rc), in_ptr)
        got_c, got_px = r.downloadReconstructedColor(), r.downloadReconstructedPixels()
    gb = r.downloadGBuffer()
    want, fill = expected_reconstruct(r, cfg, rc, in_color, gb=gb)
    assert np.array_equal(bits(got_c), bits(want)), p
    assert np.array_equal(got_px, oracle.make_color(want[..., :3].reshape(-1, 3)).reshape(got_px.shape)), p

    check_gbuffer_prim(r, gb)
    if w * h <= GBUFFER_FULL_MAX:
        gw = expected_gbuffer(oracle, model, r)
        assert np.array_equal(gb["prim"], gw["prim"])
        for k in ("position", "normal", "albedo"):
            assert np.array_equal(bits(gb[k]), bits(gw[k])), k
    r.close()


# ---- full-size reconstruction ------------------------------------------------------------------------------------------
def _check_full_size(oracle, r, cfg):
    r.render()
    r.reconstruct()
    got_c, got_px = r.downloadReconstructedColor(), r.downloadReconstructedPixels()
    gb = r.downloadGBuffer()
    want, fill = expected_reconstruct(r, cfg, gb=gb)
    assert np.array_equal(bits(got_c), bits(want))
    assert np.array_equal(got_px, oracle.make_color(want[..., :3].reshape(-1, 3)).reshape(got_px.shape))
    acc = r.downloadAccum()
    assert {1, 2, 4} <= set(np.unique(fill).tolist())
    assert not np.array_equal(got_c[fill == 4], acc[fill == 4])             # (it did reconstruct)
    check_gbuffer_prim(r, gb, rows=np.arange(0, r.launchParams.frame.size.y, 8))
    assert (gb["prim"] != 0xffffffff).mean() > 0.5


def test_reconstruct_matches_the_restatement_c3(oracle):
    """BASELINE C3: 262,144-triangle atrium at 1920 x 1080, radii 148 / 482, spp 1 / 2 / 8, defaults: 2 M G-buffer rays in
    one closest-hit launch."""
    cfg = cfg_foveated(148, 482, (1, 2, 8))
    cfg.write_guides = 1
    r = make_gpu(scenes.atrium(262144), scenes.ambient_probe(96, 54, 2.5), scenes.ATRIUM_CAMERA, (1920, 1080), cfg)
    _check_full_size(oracle, r, cfg)
    r.close()


def test_reconstruct_matches_the_restatement_c5_eye(oracle):
    """BASELINE C5, one eye: the 3.8 M-triangle atrium at 2160 x 2160 with the left eye's off-centre frustum, radii 296 / 964,
    depth 8, defaults: 4.7 M G-buffer rays in one closest-hit launch."""
    W = H = 2160
    cam = scenes.ATRIUM_CAMERA
    cfg = cfg_foveated(296, 964, (1, 2, 8), max_depth=8)
    cfg.write_guides = 1
    r = make_gpu(scenes.atrium(3800000, material="app"), scenes.ambient_probe(96, 54, 2.5), cam, (W, H), cfg)
    fwd = np.array(cam["lookat"], np.float64) - np.array(cam["eye"], np.float64)
    right = np.cross(fwd, np.array(cam["up"], np.float64))
    right /= np.linalg.norm(right)
    r.setCameraFov(tuple(np.array(cam["eye"], np.float64) - 3.2 * right), fwd, cam["up"], -0.85, 0.70, 0.78, -0.78)
    _check_full_size(oracle, r, cfg)
    r.close()


# ---- the frame as it was rendered -----------------------------------------------------------------------------------------
def _atrium(size, cfg, gaze=None):
    cfg.write_guides = 1
    return make_gpu(scenes.atrium(8000), scenes.ambient_probe(96, 54, 2.5), scenes.ATRIUM_CAMERA, size, cfg, gaze=gaze)


def _outputs(r):
    r.denoise()
    r.reconstruct()
    return [r.downloadDenoisedColor(), r.downloadDenoisedPixels(), r.downloadReconstructedColor(), r.downloadReconstructedPixels()]


def _camera(size, shift):
    cam = scenes.ATRIUM_CAMERA
    eye = (cam["eye"][0] + shift, cam["eye"][1], cam["eye"][2] + 0.5 * shift)
    return renderer.Camera(eye, cam["lookat"], cam["up"], cam["fovy"], size[0] / float(size[1]))


@pytest.mark.parametrize("change", ["gaze", "radii", "uniform", "camera"])
def test_postprocessing_uses_the_rendered_frame(change):
    """Render, then write the next gaze into launchParams, or new radii / FOV_OFF through config, or a new camera: denoise and
    reconstruct still post-process the frame as it was rendered, bit for bit what an untouched twin context gives."""
    size = (160, 90)
    cfg = cfg_foveated(15, 48, (1, 2, 8))
    r, twin = _atrium(size, cfg, gaze=(60, 40)), _atrium(size, cfg, gaze=(60, 40))
    r.render()
    twin.render()
    if change == "gaze":
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = 120, 70
    elif change == "camera":
        r.setCamera(_camera(size, 60.0))
    else:
        c = r.config
        if change == "radii":
            c.r_inner, c.r_outer = 4, 20
        else:
            c.uniform = 1
        r.config = c
    want = _outputs(twin)
    got = _outputs(r)
    for a, b in zip(got, want):
        assert np.array_equal(bits(a), bits(b)), change
    r.render()                                           # (the change matters: a frame rendered under it post-processes otherwise)
    assert not all(np.array_equal(bits(a), bits(b)) for a, b in zip(_outputs(r), want)), change
    r.close()
    twin.close()


def test_denoise_with_frames_in_flight_is_the_last_frame_issued():
    """frames_in_flight = 2: render gaze A, render gaze B without synchronising, write gaze C, denoise and reconstruct: B's frame
    post-processed, as a twin rendering A then B one at a time gives it."""
    size = (192, 108)
    gazes = [(50, 30), (140, 80)]
    cfg = cfg_foveated(15, 48, (1, 2, 8))
    cfg.frames_in_flight = 2
    r, twin = _atrium(size, cfg), _atrium(size, cfg)
    for g in gazes:
        twin.launchParams.frame.c.x, twin.launchParams.frame.c.y = g
        twin.render()
    want = _outputs(twin)
    for g in gazes:
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = g
        r.render_async()
    r.launchParams.frame.c.x, r.launchParams.frame.c.y = 20, 90
    r.denoise()
    r.reconstruct()
    r.synchronize()
    got = [r.downloadDenoisedColor(), r.downloadDenoisedPixels(), r.downloadReconstructedColor(), r.downloadReconstructedPixels()]
    for a, b in zip(got, want):
        assert np.array_equal(bits(a), bits(b))
    r.close()
    twin.close()


def test_postprocessing_follows_resizes(oracle):
    """160 x 90 -> 37 x 23 -> 200 x 120 between rendered frames: denoise and reconstruct bit for bit after each (the outputs,
    level map and G-buffer grow with the frame); after a resize nothing is left to post-process until the next render."""
    cfg = cfg_foveated(9, 30, (1, 2, 4))
    r = _atrium((160, 90), cfg)
    for k, size in enumerate([(160, 90), (37, 23), (200, 120)]):
        if k:
            r.resize(size)
            for call in (r.denoise, r.reconstruct):
                with pytest.raises(lib.FovptError) as e:
                    call()
                assert e.value.code == E_NO_FRAME
            r.setCamera(_camera(size, 0.0))
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = size[0] // 3, size[1] // 2
        r.launchParams.frame.subframe_index = 0
        r.render()
        check_denoise(oracle, r, cfg, dict(iterations_fovea=1, iterations_middle=3, iterations_periphery=5))
        check_reconstruct(oracle, r, cfg)
        check_reconstruct(oracle, r, cfg, in_color=r.downloadDenoisedColor(), in_ptr=r.denoise_buffers()[0])
    r.close()
