"""fovpt_bloom on the GPU against tests/bloom_ref.py, bit for bit: the colour, the rgba8 and every level of the pyramid over frame
sizes chosen for odd halving, clamped taps and a tile edge +- 1, every level count and flag combination and a FOV_OFF frame; the
exposure from fovpt_expose's device record; in place; the context's own buffers
across a resize; ordering with frames in flight; every rejection; a seeded sweep; the C++ drop-in; and an atrium frame through
fovpt_post -> fovpt_bloom -> fovpt_expose.  The frame description (size, passes, gaze, FOV_OFF) is the rendered one of the small box
scene; the input colour is a seeded synthetic HDR image uploaded by the tests."""
import ctypes as C
import os

import numpy as np
import pytest

import bloom_ref as br
import expose_ref as ex
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer, scenes

from common import cfg_foveated, cfg_uniform, make_gpu
from gpu_common import (bits, box_renderer, build_dropin, debug_buffer, device_images, dropin_renderer, frame_size, host_view,
                        run_dropin, upload, with_entries, writer_fills)

pytestmark = pytest.mark.gpu
E_INVALID, E_NO_FRAME = -1, -5
PROBE = scenes.ambient_probe(64, 32, 2.5)
f32 = np.float32
KARIS, GAINS, STATE = abi.BLOOM_KARIS, abi.BLOOM_GAINS, abi.BLOOM_EXPOSURE_STATE
FOUR_GAINS = dict(gain_fovea=1.0, gain_middle=0.5, gain_periphery=0.125, gain_uniform=0.75)
# threshold 1, knee 0.5 at exposure 0.25: T = 4, K = 2 -- the images below have pixels at 0, under the knee, in it and far above it
BASE = dict(FOUR_GAINS, exposure=0.25, intensity=0.2)


def radii(size):
    """Radii that put fovea, middle ring and periphery on a frame of this size (where it has the room)."""
    m = min(size)
    return max(1, m // 6), max(2, m // 3)


def bcfg(d=None):
    """fovpt_bloom_defaults with the entries of d replaced -> (abi.BloomConfig, the dict the restatement takes)."""
    c = with_entries(renderer.SampleRenderer.bloom_defaults(), d)
    return c, c.as_dict()


def hdr_image(size, seed):
    """Seeded synthetic HDR frame: 2^-6 .. 2^3 with black pixels and isolated spikes up to 2^10, alpha a ramp."""
    w, h = size
    rng = np.random.default_rng(seed)
    img = np.exp2(rng.uniform(-6, 3, (h, w, 4))).astype(np.float32)
    n = w * h
    flat = img.reshape(-1, 4)
    flat[rng.permutation(n)[:(n + 15) // 16], :3] = 0.0
    spikes = rng.permutation(n)[:(n + 23) // 24]
    flat[spikes, :3] = np.exp2(rng.uniform(4, 10, (len(spikes), 3))).astype(np.float32)
    flat[:, 3] = np.linspace(0.0, 1.0, n, dtype=np.float32)
    return img


def pyramid(r):
    """What fovpt_debug_buffer shows of the pyramid: (texels, 4) float32."""
    p, n = debug_buffer(r, "bloom_pyramid")
    assert n % 16 == 0
    return r.download(p, np.empty((n // 16, 4), np.float32))


def check(oracle, r, d, img, fill=None, in_ptr="upload", out=None, E=None, label=None):
    """One fovpt_bloom of img (uploaded; or what in_ptr holds) compared with the restatement: colour, rgba8 and the pyramid.
    fill: (fills, uniform) of the rendered frame, computed here when GAINS needs them and none are given.  out: device tensors
    (colour, rgba), None for the context's own."""
    size = frame_size(r)
    keep = upload(img) if in_ptr == "upload" else None
    cfg, full = bcfg(d)
    ptrs = (out[0].data_ptr(), out[1].data_ptr()) if out is not None else (None, None)
    r.bloom(cfg, keep.data_ptr() if keep is not None else in_ptr, *ptrs)
    if out is None:
        got_c, got_px = r.downloadBloomColor(), r.downloadBloomPixels()
    else:
        r.synchronize()
        got_c, got_px = host_view(out[0], "color"), host_view(out[1], "rgba")
    if full["flags"] & GAINS and fill is None:
        fill = writer_fills(r)
    want = br.bloom(oracle, img, full, E, *(fill if full["flags"] & GAINS else (None, 0)))
    got_pyr = pyramid(r)
    assert got_pyr.shape == want["pyramid"].shape == (br.level_offsets(size[0], size[1], full["levels"])[-1], 4), label
    off = br.level_offsets(size[0], size[1], full["levels"])
    for k in range(full["levels"]):
        assert np.array_equal(bits(got_pyr[off[k]:off[k + 1]]), bits(want["pyramid"][off[k]:off[k + 1]])), (label, "level", k)
    assert np.array_equal(bits(got_c), bits(want["color"])), label
    assert np.array_equal(got_px, want["rgba"]), label
    want["got_color"], want["got_rgba"], want["got_pyramid"] = got_c, got_px, got_pyr
    return want


# ---- 1. bit for bit ------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (2, 2), (3, 5), (17, 9), (65, 5), (64, 4), (130, 67)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_bit_for_bit(oracle, size):
    """Levels 1, 2, 5 and 8 (8 on 17 x 9 reaches 1 x 1 and keeps going) and every flag combination, each followed by a call with
    spread = 0, which leaves the d_k in the pyramid."""
    r = box_renderer(size, cfg_foveated(*radii(size), (1, 1, 2)), write_guides=True)
    r.render()
    fill = writer_fills(r)
    seen = set(np.unique(fill[0]).tolist())
    print(size, "fills", sorted(seen))
    if size == (130, 67):
        assert {1, 2, 4} <= seen                                  # fovea, middle ring and periphery all occur
    img = hdr_image(size, 11)
    acted = False
    for levels in (1, 2, 5, 8):
        for flags in (0, KARIS, GAINS, KARIS | GAINS):
            d = dict(BASE, levels=levels, flags=flags)
            want = check(oracle, r, d, img, fill, label=(size, levels, flags))
            acted |= bool((bits(want["color"]) != bits(img)).any())
            zero = check(oracle, r, dict(d, spread=0.0), img, fill, label=(size, levels, flags, "spread 0"))
            for k in range(levels):
                assert np.array_equal(bits(zero["u"][k]), bits(zero["d"][k]))
            if levels > 1 and size[0] * size[1] > 4:
                assert not np.array_equal(bits(zero["pyramid"]), bits(want["pyramid"]))
    assert acted
    if size == (17, 9):
        assert br.level_sizes(17, 9, 8)[4:] == [(1, 1)] * 4
    r.close()


def test_a_fov_off_frame_takes_gain_uniform(oracle):
    size = (37, 21)
    r = box_renderer(size, cfg_uniform(1), write_guides=True)
    r.render()
    img = hdr_image(size, 12)
    a = check(oracle, r, dict(BASE, levels=3, flags=KARIS | GAINS), img, label="fov off")
    b = check(oracle, r, dict(BASE, levels=3, flags=KARIS | GAINS, gain_uniform=0.25), img, label="fov off, another gain")
    assert not np.array_equal(bits(a["color"]), bits(b["color"]))
    # the three foveated gains play no part
    c = check(oracle, r, dict(BASE, levels=3, flags=KARIS | GAINS, gain_fovea=0.0, gain_middle=0.0, gain_periphery=0.0), img, label="fov off, others 0")
    assert np.array_equal(bits(a["color"]), bits(c["color"]))
    r.close()


# ---- 2. the exposure from fovpt_expose's device record -------------------------------------------------------------------------------
def test_exposure_state(oracle):
    """No synchronisation between the expose and the bloom calls: the exposure goes from k_expose_adapt's record into
    k_bloom_prefilter on the device."""
    size = (96, 54)
    r = box_renderer(size, cfg_foveated(*radii(size), (1, 1, 2)), write_guides=True)
    r.render()
    img = hdr_image(size, 14)
    dev = upload(img)
    d = dict(BASE, levels=4, flags=KARIS | STATE, exposure=0.25)
    out = device_images(size, 16, 4)
    before = check(oracle, r, d, img, in_ptr=dev.data_ptr(), out=out, E=0.25, label="before any AUTO step")
    assert r.expose_state().steps == 0
    ec = renderer.SampleRenderer.expose_defaults()
    ec.key = 0.5
    r.expose(ec, dev.data_ptr())
    cfg, full = bcfg(d)
    r.bloom(cfg, dev.data_ptr(), out[0].data_ptr(), out[1].data_ptr())         # behind the AUTO step, nothing in between
    st = r.expose_state()
    assert st.steps == 1 and f32(st.exposure) != f32(0.25) and 1e-3 < st.exposure < 1e3
    want = br.bloom(oracle, img, full, E=st.exposure)
    got_c, got_px = host_view(out[0], "color"), host_view(out[1], "rgba")
    assert np.array_equal(bits(got_c), bits(want["color"])) and np.array_equal(got_px, want["rgba"])
    assert np.array_equal(bits(pyramid(r)), bits(want["pyramid"]))
    assert not np.array_equal(bits(want["color"]), bits(before["color"])) and not np.array_equal(bits(want["color"]), bits(img))
    # without the flag the record is not looked at
    check(oracle, r, dict(d, flags=KARIS), img, in_ptr=dev.data_ptr(), out=out, E=0.25, label="flag off")
    r.expose_reset()
    r.bloom(cfg, dev.data_ptr(), out[0].data_ptr(), out[1].data_ptr())         # behind the reset, nothing in between
    r.synchronize()
    assert np.array_equal(bits(host_view(out[0], "color")), bits(before["color"])) and np.array_equal(host_view(out[1], "rgba"), before["rgba"])
    assert r.expose_state().steps == 0
    r.close()


# ---- 3. the buffer conventions ---------------------------------------------------------------------------------------------------------
def test_in_place_equals_out_of_place(oracle):
    size = (130, 67)
    r = box_renderer(size, cfg_foveated(*radii(size), (1, 1, 2)), write_guides=True)
    r.render()
    img = hdr_image(size, 15)
    d = dict(BASE, levels=5, flags=KARIS | GAINS)
    out = device_images(size, 16, 4)
    apart = check(oracle, r, d, img, out=out, label="out of place")
    dev = upload(img)
    same = check(oracle, r, d, img, in_ptr=dev.data_ptr(), out=(dev, out[1]), label="in place")
    assert np.array_equal(bits(same["got_color"]), bits(apart["got_color"])) and np.array_equal(same["got_rgba"], apart["got_rgba"])
    # in_color NULL is the accum buffer
    check(oracle, r, dict(d, exposure=16.0), r.downloadAccum(), in_ptr=None, out=out, label="accum")
    r.close()


def test_own_buffers_follow_a_resize(oracle):
    size = (64, 48)
    r = box_renderer(size, cfg_foveated(*radii(size), (1, 1, 2)), write_guides=True)
    with pytest.raises(lib.FovptError) as e:                 # nothing rendered yet
        r.bloom()
    assert e.value.code == E_NO_FRAME
    with pytest.raises(lib.FovptError):                      # and no pyramid was made
        debug_buffer(r, "bloom_pyramid")
    r.render()
    d = dict(BASE, levels=8, flags=KARIS | GAINS)
    check(oracle, r, d, hdr_image(size, 16), label="own buffers")
    own = r.bloomBuffers()
    assert own[0] and own[1] and own[0] != own[1]
    # caller-provided buffers leave the context's own alone
    own_c, own_px = r.downloadBloomColor(), r.downloadBloomPixels()
    check(oracle, r, dict(d, intensity=0.9), hdr_image(size, 17), out=device_images(size, 16, 4), label="caller buffers")
    assert np.array_equal(bits(own_c), bits(r.downloadBloomColor())) and np.array_equal(own_px, r.downloadBloomPixels())
    big = (150, 91)
    r.resize(big)
    r.setCamera(r.lastSetCamera)
    r.launchParams.frame.c.x, r.launchParams.frame.c.y = 70, 40
    with pytest.raises(lib.FovptError) as e:                 # nothing rendered at this size yet
        r.bloom()
    assert e.value.code == E_NO_FRAME
    r.render()
    check(oracle, r, d, hdr_image(big, 18), label="after resize")
    assert r.downloadBloomColor().shape == (91, 150, 4)
    r.close()


# ---- 4. ordering ---------------------------------------------------------------------------------------------------------------------
def test_bloom_is_ordered_with_frames_in_flight():
    """render_async, bloom, render_async, bloom of the accum buffer with no synchronisation in between: what the same sequence gives
    with a synchronise after every call."""
    import torch
    size = (384, 216)
    cfg = cfg_foveated(20, 60, (4, 8, 16))
    cfg.frames_in_flight = 2
    r = box_renderer(size, cfg, write_guides=True)
    bc, _ = bcfg(dict(FOUR_GAINS, flags=KARIS | GAINS, threshold=0.5, intensity=0.5))
    views = [((190, 108), 0), ((300, 40), 1), ((80, 60), 2)]
    outs = [[device_images(size, 16, 4) for _ in views] for _ in range(2)]
    for sync, out in zip((True, False), outs):
        for g, k in views:                                   # the accum buffer's leftovers where no pass writes, as all views leave them
            r.launchParams.frame.c.x, r.launchParams.frame.c.y = g
            r.launchParams.frame.subframe_index = k
            r.render()
        for (g, k), (oc, op) in zip(views, out):
            r.launchParams.frame.c.x, r.launchParams.frame.c.y = g
            r.launchParams.frame.subframe_index = k
            r.render_async()
            if sync:
                r.synchronize()
            r.bloom(bc, None, oc.data_ptr(), op.data_ptr())
            if sync:
                r.synchronize()
        r.synchronize()
    for want, got in zip(*outs):
        for x, y in zip(want, got):
            assert torch.equal(x, y)
    a, b = host_view(outs[0][0][1], "rgba"), host_view(outs[0][2][1], "rgba")
    assert (a != b).mean() > 0.1                             # (the frames differ: the comparison is not of copies)
    accum = r.downloadAccum()
    assert (bits(host_view(outs[0][2][0], "color")) != bits(accum)).any()          # and the stage acted on them
    r.close()


# ---- 5. rejections -------------------------------------------------------------------------------------------------------------------
def _bad_configs():
    nan, inf = float("nan"), float("inf")
    up = float(np.nextafter(f32(1), f32(2)))
    out = [("flags", dict(flags=8)), ("flags", dict(flags=-1)), ("flags", dict(flags=KARIS | 16)), ("levels", dict(levels=0)), ("levels", dict(levels=9)),
           ("levels", dict(levels=-1))]
    for k in ("threshold", "exposure"):
        out += [(k, {k: v}) for v in (0.0, -1.0, nan, inf, abi.SIGMA_MIN / 2, abi.SIGMA_MAX * 2)]
    for k in ("knee", "intensity"):
        out += [(k, {k: v}) for v in (-1.0, -1e-30, nan, inf, abi.SIGMA_MAX * 2)]
    for k in ("spread", "gain_fovea", "gain_middle", "gain_periphery", "gain_uniform"):
        out += [(k, {k: v}) for v in (-0.5, -1e-30, nan, inf, up, 2.0)]
    return out


def test_rejections_leave_everything_unchanged(oracle):
    """Every FOVPT_E_INVALID case of the header and FOVPT_E_NO_FRAME, each leaving the outputs, the pyramid and the exposure state
    byte for byte.  (Not here: width * height >= 2^31, which needs a rendered frame of 32 GiB.)"""
    size = (64, 48)
    r = box_renderer(size, cfg_foveated(*radii(size), (1, 1, 2)), write_guides=True)
    L = lib.load()
    r.render()
    img = hdr_image(size, 19)
    dev = upload(img)
    ec = renderer.SampleRenderer.expose_defaults()
    r.expose(ec, dev.data_ptr())
    caller = device_images(size, 16, 4)
    good = dict(BASE, levels=5, flags=KARIS | GAINS | STATE)
    check(oracle, r, good, img, in_ptr=dev.data_ptr(), out=caller, E=r.expose_state().exposure, label="a valid call into caller's buffers")
    check(oracle, r, good, img, in_ptr=dev.data_ptr(), E=r.expose_state().exposure, label="a valid call")

    def everything():
        return (bytes(r.expose_state()), r.downloadBloomColor().tobytes(), r.downloadBloomPixels().tobytes(), pyramid(r).tobytes(),
                caller[0].cpu().numpy().tobytes(), caller[1].cpu().numpy().tobytes(), dev.cpu().numpy().tobytes())

    before = everything()

    def refuse(code, label, call):
        with pytest.raises(lib.FovptError) as e:
            call()
        assert e.value.code == code, label
        assert everything() == before, label

    for label, d in _bad_configs():
        c, _ = bcfg(dict(good, **d))
        refuse(E_INVALID, (label, d), lambda: r.bloom(c, dev.data_ptr()))
    for i in range(5):
        c, _ = bcfg(good)
        c._reserved[i] = 1
        refuse(E_INVALID, "_reserved[%d]" % i, lambda: r.bloom(c, dev.data_ptr()))
    c, _ = bcfg(good)
    assert L.fovpt_bloom(r._ctx, None, C.byref(c), None, None, None) == E_INVALID
    assert L.fovpt_bloom(r._ctx, C.byref(r.launchParams), None, None, None, None) == E_INVALID
    assert L.fovpt_bloom(None, C.byref(r.launchParams), C.byref(c), None, None, None) == E_INVALID
    col_, rgba_ = C.c_void_p(), C.c_void_p()
    assert L.fovpt_bloom_buffers(r._ctx, None, C.byref(rgba_)) == E_INVALID and L.fovpt_bloom_buffers(r._ctx, C.byref(col_), None) == E_INVALID
    assert everything() == before
    # aliases: an output that is the pyramid or the other output; the rgba output or the pyramid as the input
    pyr = debug_buffer(r, "bloom_pyramid")[0]
    oc, op = caller[0].data_ptr(), caller[1].data_ptr()
    refuse(E_INVALID, "out_color is the pyramid", lambda: r.bloom(c, dev.data_ptr(), pyr, op))
    refuse(E_INVALID, "out_rgba is the pyramid", lambda: r.bloom(c, dev.data_ptr(), oc, pyr))
    refuse(E_INVALID, "out_color is out_rgba", lambda: r.bloom(c, dev.data_ptr(), oc, oc))
    refuse(E_INVALID, "out_rgba is the input", lambda: r.bloom(c, dev.data_ptr(), oc, dev.data_ptr()))
    refuse(E_INVALID, "the input is the pyramid", lambda: r.bloom(c, pyr, oc, op))
    f = r.launchParams.frame
    f.size.x -= 4
    with pytest.raises(lib.FovptError) as e:
        r.bloom(c, dev.data_ptr())
    f.size.x += 4                                            # (the downloads of everything() go by this size)
    assert e.value.code == E_NO_FRAME and everything() == before
    keep = f.accum_buffer
    f.accum_buffer = None
    refuse(E_INVALID, "null accum_buffer", lambda: r.bloom(c))
    f.accum_buffer = keep
    cf = r.config                                            # a tile shard does not see the frame
    cf.world, cf.rank = 2, 0
    r.config = cf
    r.render()
    refuse(E_INVALID, "world 2", lambda: r.bloom(c, dev.data_ptr()))
    cf.world, cf.rank = 1, 0
    r.config = cf
    r.render()
    check(oracle, r, good, img, in_ptr=dev.data_ptr(), E=r.expose_state().exposure, label="the valid call after them")
    assert everything() == before
    r.close()


# ---- 6. a seeded sweep ---------------------------------------------------------------------------------------------------------------
def _random_config(rng):
    d = dict(flags=int(rng.integers(0, 4)), levels=int(rng.integers(1, 9)), threshold=float(f32(np.exp2(rng.uniform(-3, 3)))),
             knee=float(f32(rng.choice([0.0, np.exp2(rng.uniform(-4, 2))]))), exposure=float(f32(np.exp2(rng.uniform(-6, 4)))),
             intensity=float(f32(rng.choice([0.0, np.exp2(rng.uniform(-8, 2))]))), spread=float(f32(rng.choice([0.0, 1.0, rng.uniform(0, 1)]))))
    for k in ("gain_fovea", "gain_middle", "gain_periphery", "gain_uniform"):
        d[k] = float(f32(rng.choice([0.0, 1.0, rng.uniform(0, 1)])))
    return d


@pytest.mark.parametrize("seed", range(int(os.environ.get("FOVPT_FUZZB_TO", "24"))))
def test_seeded_sweep(oracle, seed):
    rng = np.random.default_rng(3000 + seed)
    w, h = int(rng.integers(1, 97)), int(rng.integers(1, 97))
    uniform = rng.random() < 0.25
    ri = int(rng.integers(0, 12))
    cfg = cfg_uniform(1) if uniform else cfg_foveated(ri, ri + int(rng.integers(0, 24)), (1, 1, 1))
    gaze = (int(rng.integers(-8, w + 8)) & 0xffffffff, int(rng.integers(-8, h + 8)) & 0xffffffff)
    r = box_renderer((w, h), cfg, gaze, write_guides=True)
    r.render()
    fill = writer_fills(r)
    for k in range(2):
        d = _random_config(rng)
        print(seed, k, (w, h), d)
        check(oracle, r, d, hdr_image((w, h), 4000 + 2 * seed + k), fill, label=(seed, k))
    r.close()


# ---- 7. the C++ drop-in ----------------------------------------------------------------------------------------------------------------
def test_cpp_dropin_bloom(tmp_path):
    """SampleRenderer::bloomPost() / bloom() / exposeBloom() of include/SimplePathtracer.h: the same bytes as Python."""
    exe, out = build_dropin(tmp_path, "bloom_gpu_test"), str(tmp_path / "bloom_out.bin")
    run_dropin(exe, out)
    n = 160 * 96
    raw = np.fromfile(out, np.uint32)
    assert raw.size == 2 * 4 * n + 3 * n
    color = raw[:8 * n].reshape(2, 96, 160, 4)
    px = raw[8 * n:].reshape(3, 96, 160)
    r = dropin_renderer(write_guides=True)
    r.render()
    r.post()
    bc, _ = bcfg(dict(flags=KARIS | GAINS, levels=5, threshold=0.5, exposure=1.0, intensity=0.25, gain_fovea=1.0, gain_middle=0.5, gain_periphery=0.25))
    r.bloom(bc, r.post_buffers()[0])
    assert np.array_equal(color[0], bits(r.downloadBloomColor())) and np.array_equal(px[0], r.downloadBloomPixels())
    assert (color[0] != bits(r.downloadPostColor())).any()
    ec = renderer.SampleRenderer.expose_defaults()
    ec.mode, ec.exposure = abi.EXPOSE_FIXED, 2.0
    r.expose(ec, r.bloomBuffers()[0])
    assert np.array_equal(px[1], r.downloadExposedPixels())
    r.bloom()
    assert np.array_equal(color[1], bits(r.downloadBloomColor())) and np.array_equal(px[2], r.downloadBloomPixels())
    assert len(np.unique(px[0])) > 20
    r.close()


# ---- 8. the atrium through post -> bloom -> expose ---------------------------------------------------------------------------------
def test_the_atrium_through_post_bloom_expose(oracle):
    """One 384 x 216 frame of a scene with depth complexity through the chain as an application runs it, each stage
    into the context's own buffers and the next one reading them, nothing synchronised in between.  The restatements are chained
    the same way from the colour fovpt_post left (which has its own restatement: test_post_gpu.py)."""
    size = (384, 216)
    cf = cfg_foveated(40, 100, (1, 1, 2))
    cf.write_guides = 1
    r = make_gpu(scenes.atrium(8000), PROBE, scenes.ATRIUM_CAMERA, size, cf)
    r.render()
    r.post()
    bc, bfull = bcfg(dict(FOUR_GAINS, flags=KARIS | GAINS, threshold=0.75, intensity=0.3))
    r.bloom(bc, r.post_buffers()[0])
    ec = renderer.SampleRenderer.expose_defaults()
    r.expose(ec, r.bloomBuffers()[0])
    post = r.downloadPostColor()
    want_b = br.bloom(oracle, post, bfull, None, *writer_fills(r))
    assert np.array_equal(bits(r.downloadBloomColor()), bits(want_b["color"])) and np.array_equal(r.downloadBloomPixels(), want_b["rgba"])
    assert np.array_equal(bits(pyramid(r)), bits(want_b["pyramid"]))
    changed = (bits(want_b["color"]) != bits(post)).any(axis=-1).mean()
    print("atrium: pixels the bloom changed", changed, "pyramid maximum", float(want_b["pyramid"].max()))
    assert changed > 0.1
    want_c, want_px, _, state = ex.expose(oracle, want_b["color"], ec.as_dict(), ex.new_state(), *writer_fills(r))
    assert np.array_equal(bits(r.downloadExposedColor()), bits(want_c)) and np.array_equal(r.downloadExposedPixels(), want_px)
    assert r.expose_state().steps == 1 and f32(r.expose_state().exposure) == f32(state["exposure"])
    r.close()
