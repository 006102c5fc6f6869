"""fovpt_expose on the GPU against tests/expose_ref.py, bit for bit: the anchor (today's tone map), the histogram on edge values
and every metering mode, a frame of many blocks, adaptation over steps and the reset paths, nothing to meter, both operators and
the buffer conventions, ordering with frames in flight, the buffers it must leave alone, every rejection, a seeded sweep, and the
C++ drop-in.  Inputs are synthetic frames uploaded by the tests; the frame description (passes, gaze, FOV_OFF) is the rendered one."""
import ctypes as C
import os

import numpy as np
import pytest

import expose_ref as ex
from fovpathtracing_optixcodelatest_amd import abi, lib, scenes

from common import cfg_foveated, cfg_uniform, make_gpu
from gpu_common import bits, build_dropin, debug_buffer, dropin_renderer, run_dropin, upload, with_entries, writer_fills

pytestmark = pytest.mark.gpu
E_INVALID, E_NO_FRAME = -1, -5
CORNELL = scenes.CORNELL_CAMERA
PROBE = scenes.ambient_probe(64, 32, 2.0)
SIZE = (64, 48)
f32 = np.float32
DENORMAL = float(np.uint32(1).view(np.float32))
EDGES = [2.0 ** -17, 2.0 ** -16, 1.0, 65535.0, 2.0 ** 20, np.inf, np.nan, 0.0, -1.0, DENORMAL]


def _cornell(size=SIZE, cfg=None, gaze=None):
    cfg = cfg if cfg is not None else cfg_foveated(6, 14, (1, 1, 2))
    cfg.write_guides = 1
    return make_gpu(scenes.cornell_box(), PROBE, CORNELL, size, cfg, gaze=gaze)


def ecfg(d):
    """fovpt_expose_defaults with the entries of d replaced -> (abi.ExposeConfig, the full dict for the restatement)."""
    c = abi.ExposeConfig()
    lib.check(None, lib.load().fovpt_expose_defaults(c))
    return with_entries(c, d), c.as_dict()


def histogram(r):
    p, n = debug_buffer(r, "expose_histogram")
    assert n == 256 * 8
    return r.download(p, np.empty(256, np.uint64))


def same_state(got, want, label=None):
    for k in ("ev_metered", "ev", "exposure"):
        assert f32(getattr(got, k)).view(np.uint32) == f32(want[k]).view(np.uint32), (label, k, getattr(got, k), want[k])
    assert got.weight_total == want["weight_total"] and got.steps == want["steps"], (label, got.weight_total, got.steps, want)


def usable(inp):
    """The pixels whose outputs are specified: finite and non-negative in all three channels."""
    c = inp[..., :3]
    with np.errstate(invalid="ignore"):
        return (np.isfinite(c) & (c >= 0)).all(axis=-1)


class Checker:
    """Follows one renderer's exposure state: every step() is compared with the restatement (outputs where they are specified,
    the histogram and the state record)."""

    def __init__(self, oracle, r):
        self.oracle, self.r, self.state = oracle, r, ex.new_state()

    def reset(self):
        self.state = ex.new_state()

    def step(self, d, inp, in_ptr="upload", out=None, label=None):
        r = self.r
        f = r.launchParams.frame
        shape = (f.size.y, f.size.x)
        keep = upload(inp) if in_ptr == "upload" else None
        c, full = ecfg(d)
        r.expose(c, keep.data_ptr() if keep is not None else in_ptr, *(out or (None, None)))
        if out is None:
            got_c, got_px = r.downloadExposedColor(), r.downloadExposedPixels()
        else:
            got_c, got_px = r.download(out[0], np.empty(shape + (4,), np.float32)), r.download(out[1], np.empty(shape, np.uint32))
        fill, uniform = writer_fills(r) if full["metering"] == ex.GAZE and full["mode"] == ex.AUTO else (None, 0)
        want_c, want_px, want_h, self.state = ex.expose(self.oracle, inp, full, self.state, fill, uniform)
        if want_h is not None:
            assert np.array_equal(histogram(r), want_h), label
        if self.state["steps"]:
            same_state(r.expose_state(), self.state, label)
        ok = usable(inp)
        assert np.array_equal(bits(got_c[ok]), bits(want_c[ok])), label
        assert np.array_equal(got_px[ok], want_px[ok]), label
        return dict(color=got_c, rgba=got_px, hist=want_h, fill=fill, ok=ok)


def edge_frame(w, h, seed):
    """Every edge value in the frame (as its luminance: grey pixels), the rest log-uniform over 2^-20 .. 2^20."""
    rng = np.random.default_rng(seed)
    L = np.exp2(rng.uniform(-20, 20, (h, w))).astype(np.float32)
    spots = rng.permutation(w * h)
    for k in range(min(w * h, 3 * len(EDGES))):
        L.reshape(-1)[spots[k]] = EDGES[k % len(EDGES)]
    img = np.repeat(L[..., None], 4, axis=-1)
    img[..., 3] = 1.0
    return img


# ---- 1. the anchor ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("uniform", [False, True], ids=["foveated", "fov_off"])
def test_fixed_16_reinhard_1_is_the_resolves_rgba8(oracle, uniform):
    """The resolve's frame_buffer wherever a pass writes it (a FOV_OFF frame: everywhere; the foveated 64 x 48 frame leaves one
    pixel between the rings that no pass writes, where frame_buffer keeps fovpt_resize's 0 and accum its zeros), and the oracle's
    tone map of the accum buffer everywhere."""
    r = _cornell(cfg=cfg_uniform(2) if uniform else None)
    r.render()
    c, _ = ecfg(dict(mode=abi.EXPOSE_FIXED, exposure=16.0, tone=abi.TONE_REINHARD, white=1.0))
    r.expose(c)
    got = r.downloadExposedPixels()
    accum = r.downloadAccum()
    written = writer_fills(r)[0] > 0
    assert written.all() if uniform else (~written).sum() == 1
    assert np.array_equal(got[written], r.downloadPixels()[written])
    assert not accum[~written].any() and (r.downloadPixels()[~written] == 0).all()
    assert np.array_equal(got.reshape(-1), oracle.make_color(accum[..., :3].reshape(-1, 3)))
    assert len(np.unique(got)) > 20                           # (a picture, not a constant)
    col = r.downloadExposedColor()
    assert (col[..., 3] == 1).all()
    assert r.expose_state().steps == 0                        # FIXED: no state, and none is made
    with pytest.raises(lib.FovptError):
        debug_buffer(r, "expose_state")
    r.close()


# ---- 2. the histogram -----------------------------------------------------------------------------------------------------------------
def test_the_histogram_on_edge_values(oracle):
    size = (61, 37)
    r = _cornell(size)
    ck = Checker(oracle, r)
    img = edge_frame(size[0], size[1], 1)
    seen = set()
    cases = [("in the frame", (30, 18), False), ("at a corner", (0, 0), False), ("at the last pixel", (60, 36), False),
             ("off the frame", (61 + 40, 37 + 40), False), ("far off the frame", (4000, 3000), False), ("FOV_OFF", (30, 18), True)]
    for label, gaze, uniform in cases:
        cfg = cfg_uniform(1) if uniform else cfg_foveated(6, 14, (1, 1, 2))
        cfg.write_guides = 1
        r.config = cfg
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = gaze
        r.render()
        for d in (dict(metering=abi.METER_FRAME), dict(metering=abi.METER_GAZE, weight_fovea=255, weight_middle=9, weight_periphery=2, weight_uniform=5),
                  dict(metering=abi.METER_GAZE, weight_middle=0), dict(metering=abi.METER_GAZE, weight_periphery=0, weight_uniform=0)):
            ck.reset()
            r.expose_reset()
            o = ck.step(dict(d, ev_min=-16.0, ev_max=16.0), img, label=(label, d))
            if o["fill"] is not None:
                seen |= set(np.unique(o["fill"]).tolist())
            if d["metering"] == abi.METER_FRAME:
                assert o["hist"][0] >= 9 and o["hist"][255] >= 9 and o["hist"].sum() == size[0] * size[1] - 9      # (NaN, 0 and -1 do not count)
    assert {0, 1, 2, 4} <= seen                              # (0: the pixels no pass writes)
    r.close()


@pytest.mark.parametrize("size", [(1, 1), (3, 1), (1, 5), (4, 4)], ids=lambda s: "%dx%d" % s)
def test_the_histogram_of_tiny_frames(oracle, size):
    r = _cornell(size, cfg_foveated(1, 2, (1, 1, 1)), gaze=(0, 0))
    ck = Checker(oracle, r)
    r.render()
    for k, v in enumerate((1.0, 65535.0, np.nan)):
        img = np.full((size[1], size[0], 4), v, np.float32)
        img[0, 0, :3] = 3.0
        for d in (dict(metering=abi.METER_FRAME), dict(metering=abi.METER_GAZE, weight_fovea=3, weight_middle=2)):
            ck.step(d, img, label=(size, v, d))
    cfg = cfg_uniform(1)
    r.config = cfg
    r.render()
    ck.step(dict(metering=abi.METER_GAZE, weight_uniform=7), np.full((size[1], size[0], 4), 0.25, np.float32))
    assert r.expose_state().weight_total == 7 * size[0] * size[1]
    r.close()


# ---- 3. many blocks -------------------------------------------------------------------------------------------------------------------
def test_a_frame_of_many_blocks(oracle):
    size = (1920, 1080)
    r = _cornell(size, cfg_foveated(74, 241, (1, 1, 1)), gaze=(1000, 500))
    r.render()
    rng = np.random.default_rng(7)
    img = np.exp2(rng.normal(0.0, 4.0, (size[1], size[0], 4))).astype(np.float32)
    ck = Checker(oracle, r)
    o = ck.step(None, img)                                    # the defaults: AUTO, GAZE
    assert (o["hist"] > 0).sum() > 100 and {1, 2, 4} <= set(np.unique(o["fill"]).tolist())
    assert r.expose_state().weight_total == int(ex.weights(o["fill"], ex.DEFAULTS, 0).sum()) > size[0] * size[1]
    r.close()


# ---- 4. adaptation and the reset paths ------------------------------------------------------------------------------------------------
def test_adaptation_over_steps_and_the_reset_paths(oracle):
    r = _cornell()
    ck = Checker(oracle, r)
    r.render()
    rng = np.random.default_rng(3)
    base = np.exp2(rng.normal(0.0, 1.5, (SIZE[1], SIZE[0], 4))).astype(np.float32)
    rates = [(1.0, 1.0), (0.5, 0.25), (0.125, 1.0), (0.3, 0.7), (0.8, 0.01), (0.9, 0.9)]      # (a rate of 1 lands on the target: only the first)
    evs = []
    for k, (up, down) in enumerate(rates):
        img = (base * f32(64.0 if k % 2 == 0 else 1.0 / 64.0)).astype(np.float32)
        ck.step(dict(adapt_brighter=up, adapt_darker=down, metering=k % 2), img, label=k)
        evs.append(float(r.expose_state().ev))
    st = r.expose_state()
    assert st.steps == 6 and len(set(evs)) == 6 and st.ev != st.ev_metered
    r.expose_reset()
    ck.reset()
    assert r.expose_state().steps == 0
    ck.step(dict(adapt_brighter=0.5, adapt_darker=0.5), base, label="after reset")
    st = r.expose_state()
    assert st.steps == 1 and st.ev == st.ev_metered
    # the state survives fovpt_resize
    r.resize((40, 24))
    r.setCamera(r.lastSetCamera)
    r.launchParams.frame.c.x, r.launchParams.frame.c.y = 20, 12
    with pytest.raises(lib.FovptError) as e:                 # (nothing rendered at this size yet)
        r.expose()
    assert e.value.code == E_NO_FRAME
    r.render()
    small = (base[:24, :40] * f32(32.0)).astype(np.float32)
    ck.step(dict(adapt_brighter=0.5, adapt_darker=0.5), small, label="after resize")
    st = r.expose_state()
    assert st.steps == 2 and st.ev != st.ev_metered
    assert debug_buffer(r, "expose_state")[1] == 32
    # and fovpt_set_probe; fovpt_set_scene resets it
    from fovpathtracing_optixcodelatest_amd import renderer
    r.setProbe(renderer.ProbeData(scenes.ambient_probe(32, 16, 1.0)).BuildCDF())
    assert r.expose_state().steps == 2
    from test_temporal_gpu import _scene_again
    _scene_again(r)
    assert r.expose_state().steps == 0
    ck.reset()
    r.render()
    ck.step(dict(adapt_brighter=0.5, adapt_darker=0.5), small, label="after set_scene")
    assert r.expose_state().steps == 1
    r.close()


# ---- 5. nothing to meter --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["black", "nan"])
def test_nothing_to_meter(oracle, what):
    r = _cornell()
    ck = Checker(oracle, r)
    r.render()
    empty = np.full((SIZE[1], SIZE[0], 4), 0.0 if what == "black" else np.nan, np.float32)
    lit = np.full((SIZE[1], SIZE[0], 4), 5.0, np.float32)
    ck.step(dict(ev_min=1.5, ev_max=4.0), empty, label="first step")
    st = r.expose_state()
    assert (st.ev, st.ev_metered, st.weight_total, st.steps) == (1.5, 1.5, 0, 1)
    ck.step(None, lit, label="lit")
    ev = r.expose_state().ev
    ck.step(dict(adapt_brighter=0.5, adapt_darker=0.5, ev_min=-1.0, ev_max=1.0), empty, label="later step")
    st = r.expose_state()
    assert (st.ev, st.ev_metered, st.weight_total, st.steps) == (ev, ev, 0, 3) and ev > 2
    # all weights 0 is nothing to meter too
    ck.step(dict(weight_fovea=0, weight_middle=0, weight_periphery=0), lit, label="no weight")
    assert r.expose_state().weight_total == 0 and r.expose_state().ev == ev
    r.close()


# ---- 6. the operators and the buffer conventions --------------------------------------------------------------------------------------
@pytest.mark.parametrize("tone", [abi.TONE_REINHARD, abi.TONE_ACES], ids=["reinhard", "aces"])
def test_the_operators_bit_for_bit(oracle, tone):
    import torch
    r = _cornell()
    ck = Checker(oracle, r)
    r.render()
    rng = np.random.default_rng(11 + tone)
    h, w = SIZE[1], SIZE[0]
    img = np.exp2(rng.uniform(-12, 8, (h, w, 4))).astype(np.float32)
    img.reshape(-1, 4)[rng.permutation(w * h)[:200], :3] = 0.0                       # black pixels are specified too
    for white in (1.0, 1e6, 3.5):
        for d in (dict(mode=abi.EXPOSE_FIXED, exposure=16.0), dict(mode=abi.EXPOSE_FIXED, exposure=0.37), dict(mode=abi.EXPOSE_AUTO, key=0.5)):
            o = ck.step(dict(d, tone=tone, white=white), img, label=(white, d))       # the context's own buffers
            assert o["ok"].all() and len(np.unique(o["rgba"])) > 100
        if tone == abi.TONE_ACES:
            break                                                                     # (white is REINHARD's)
    # caller-provided buffers; the context's own keep their bytes
    own_c, own_px = r.downloadExposedColor(), r.downloadExposedPixels()
    oc = torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda")
    op = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    o = ck.step(dict(tone=tone, key=0.3), img, out=(oc.data_ptr(), op.data_ptr()), label="caller buffers")
    assert np.array_equal(bits(own_c), bits(r.downloadExposedColor())) and np.array_equal(own_px, r.downloadExposedPixels())
    assert not np.array_equal(o["rgba"], own_px)
    # out_color == in_color: the meter reads the input before any pixel is written
    dev = upload(img)
    o2 = ck.step(dict(tone=tone, key=0.3, adapt_brighter=0.5, adapt_darker=0.5), img, in_ptr=dev.data_ptr(), out=(dev.data_ptr(), op.data_ptr()),
                 label="in place")
    assert np.array_equal(bits(o2["color"]), bits(o["color"]))                        # (the same input, the same ev: no movement)
    # in_color NULL is the accum buffer
    ck.step(dict(tone=tone), r.downloadAccum(), in_ptr=None, label="accum")
    r.close()


# ---- 7. ordering ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["frames_in_flight", "chains_per_frame"])
def test_expose_is_ordered_with_frames_in_flight(mode):
    """render_async, expose, render_async, expose of the accum buffer with no synchronisation in between: what the same sequence
    gives with a synchronise after every call."""
    import torch
    size = (384, 216)
    cfg = cfg_foveated(20, 60, (4, 8, 16))               # >= 16384 sample slots: chains_per_frame = 2 does split the frame
    if mode == "frames_in_flight":
        cfg.frames_in_flight = 2
    else:
        cfg.chains_per_frame = 2
    r = _cornell(size, cfg)
    c, _ = ecfg(dict(adapt_brighter=0.5, adapt_darker=0.5, key=0.4))
    views = [((120, 90), 0), ((300, 40), 1), ((30, 200), 2)]
    outs = [[(torch.empty((size[1], size[0], 4), dtype=torch.float32, device="cuda"), torch.empty((size[1], size[0]), dtype=torch.int32, device="cuda"))
             for _ in views] for _ in range(2)]
    torch.cuda.synchronize()
    states = []

    def setup(g, k):
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = g
        r.launchParams.frame.subframe_index = k

    for sync, out in zip((True, False), outs):
        for g, k in views:                                   # the accum buffer's leftovers where no pass writes, as all views leave them
            setup(g, k)
            r.render()
        r.expose_reset()
        for (g, k), (oc, op) in zip(views, out):
            setup(g, k)
            r.render_async()
            if sync:
                r.synchronize()
            r.expose(c, None, oc.data_ptr(), op.data_ptr())
            if sync:
                r.synchronize()
        r.synchronize()
        states.append(bytes(r.expose_state()))
    for want, got in zip(*outs):
        for x, y in zip(want, got):
            assert np.array_equal(x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32))
    assert states[0] == states[1] and r.expose_state().steps == 3
    a, b = outs[0][0][1].cpu().numpy(), outs[0][2][1].cpu().numpy()
    assert (a != b).mean() > 0.1                             # (the frames differ: the comparison is not of copies)
    r.close()


# ---- 8. isolation ---------------------------------------------------------------------------------------------------------------------
def test_expose_leaves_the_other_stages_buffers_alone():
    size = (96, 64)
    a, b = (_cornell(size, cfg_foveated(10, 24, (1, 2, 4))) for _ in range(2))
    for r in (a, b):
        r.render()
        r.denoise()
        r.reconstruct()
        r.temporal()
        r.post()

    def snapshot(r):
        out = [r.downloadPostColor(), r.downloadPostPixels(), r.downloadDenoisedColor(), r.downloadDenoisedPixels(), r.downloadReconstructedColor(),
               r.downloadReconstructedPixels(), r.downloadTemporalColor(), r.downloadTemporalPixels(), r.downloadTemporalHistory(), r.downloadAccum(),
               r.downloadPixels()]
        g = r.gbuffer()                                       # (traced again by both contexts: the same rays)
        return out + [r.download(getattr(g, k), np.empty((size[1], size[0], 4), np.float32)) for k in ("position", "normal", "albedo")]

    before = snapshot(b)
    b.expose(None, b.post_buffers()[0])
    b.expose(ecfg(dict(metering=abi.METER_FRAME, tone=abi.TONE_ACES))[0], b.post_buffers()[0])
    after = snapshot(b)
    for x, y in zip(before, after):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert (bits(b.downloadExposedColor()) != bits(b.downloadPostColor())).any()
    for k in range(2):                                       # the next steps equal those of the context that never exposed
        for r in (a, b):
            r.launchParams.frame.c.x += 9
            r.render()
            r.post()
        b.expose(None, b.post_buffers()[0])
        assert np.array_equal(bits(a.downloadPostColor()), bits(b.downloadPostColor())) and np.array_equal(a.downloadPostPixels(), b.downloadPostPixels())
        assert np.array_equal(bits(a.downloadTemporalHistory()), bits(b.downloadTemporalHistory()))
    with pytest.raises(lib.FovptError):                      # and that context never made exposure buffers
        debug_buffer(a, "expose_histogram")
    for r in (a, b):
        r.close()


# ---- 9. rejections --------------------------------------------------------------------------------------------------------------------
def _bad_configs():
    nan, inf = float("nan"), float("inf")
    out = [("mode", dict(mode=2)), ("mode", dict(mode=-1)), ("metering", dict(metering=2)), ("metering", dict(metering=-1)), ("tone", dict(tone=2)),
           ("tone", dict(tone=-1)), ("_reserved0", dict(_reserved0=1))]
    for k in ("weight_fovea", "weight_middle", "weight_periphery", "weight_uniform"):
        out += [(k, {k: v}) for v in (-1, 256, 1 << 30)]
    out += [("permille", dict(low_permille=lo, high_permille=hi)) for lo, hi in ((-1, 500), (500, 500), (600, 500), (0, 1001), (1000, 1000))]
    out += [("ev", dict(ev_min=lo, ev_max=hi)) for lo, hi in ((-16.5, 0.0), (0.0, 16.5), (1.0, 0.5), (nan, 1.0), (-1.0, nan), (-inf, 0.0), (0.0, inf))]
    for k in ("key", "exposure", "white"):
        out += [(k, {k: v}) for v in (0.0, -1.0, nan, inf, abi.SIGMA_MIN / 2, abi.SIGMA_MAX * 2)]
    for k in ("adapt_brighter", "adapt_darker"):
        out += [(k, {k: v}) for v in (0.0, -0.5, nan, inf, float(np.nextafter(f32(1), f32(2))))]
    return out


def test_rejections_leave_everything_unchanged(oracle):
    r = _cornell()
    with pytest.raises(lib.FovptError) as e:                 # nothing rendered yet
        r.expose()
    assert e.value.code == E_NO_FRAME
    r.render()
    ck = Checker(oracle, r)
    img = edge_frame(SIZE[0], SIZE[1], 9)
    ck.step(dict(adapt_brighter=0.5, adapt_darker=0.5), img)
    ck.step(dict(adapt_brighter=0.5, adapt_darker=0.5), (img * f32(8)).astype(np.float32))

    def everything():
        return bytes(r.expose_state()), r.downloadExposedColor().tobytes(), r.downloadExposedPixels().tobytes(), histogram(r).tobytes()

    before = everything()
    L = lib.load()

    def refuse(code, label, call):
        with pytest.raises(lib.FovptError) as e:
            call()
        assert e.value.code == code, label
        assert everything() == before, label

    for label, d in _bad_configs():
        c, _ = ecfg({k: v for k, v in d.items() if k != "_reserved0"})
        if "_reserved0" in d:
            c._reserved0 = 1
        for mode in (abi.EXPOSE_AUTO, abi.EXPOSE_FIXED):
            if "mode" not in d:
                c.mode = mode
            refuse(E_INVALID, (label, d, mode), lambda: r.expose(c))
    for i in range(3):
        c, _ = ecfg(None)
        c._reserved[i] = 1
        refuse(E_INVALID, "_reserved[%d]" % i, lambda: r.expose(c))
    good, _ = ecfg(None)
    assert L.fovpt_expose(r._ctx, None, C.byref(good), None, None, None) == E_INVALID
    assert L.fovpt_expose(r._ctx, C.byref(r.launchParams), None, None, None, None) == E_INVALID
    col_, rgba_ = C.c_void_p(), C.c_void_p()
    assert L.fovpt_expose_buffers(r._ctx, None, C.byref(rgba_)) == E_INVALID and L.fovpt_expose_buffers(r._ctx, C.byref(col_), None) == E_INVALID
    assert L.fovpt_expose_state(r._ctx, None) == E_INVALID
    assert everything() == before
    f = r.launchParams.frame
    f.size.x -= 4
    with pytest.raises(lib.FovptError) as e:
        r.expose()
    f.size.x += 4                                            # (the downloads of everything() go by this size)
    assert e.value.code == E_NO_FRAME and everything() == before
    keep = f.accum_buffer
    f.accum_buffer = None
    refuse(E_INVALID, "null accum_buffer", lambda: r.expose())
    f.accum_buffer = keep
    c = r.config                                             # a tile shard does not see the frame
    c.world, c.rank = 2, 0
    r.config = c
    r.render()
    refuse(E_INVALID, "world 2", lambda: r.expose())
    c.world, c.rank = 1, 0
    r.config = c
    r.render()
    ck.step(dict(adapt_brighter=0.5, adapt_darker=0.5), img, label="the valid step after them")
    assert r.expose_state().steps == 3
    r.close()


# ---- 10. a seeded sweep ---------------------------------------------------------------------------------------------------------------
def _random_config(rng):
    lo = int(rng.integers(0, 1000))
    ev = np.sort(rng.uniform(-16, 16, 2)).astype(np.float32)
    d = dict(mode=int(rng.random() < 0.85), metering=int(rng.integers(0, 2)), tone=int(rng.integers(0, 2)),
             low_permille=lo, high_permille=int(rng.integers(lo + 1, 1001)), ev_min=float(ev[0]), ev_max=float(ev[1]),
             key=float(f32(np.exp2(rng.uniform(-8, 8)))), exposure=float(f32(np.exp2(rng.uniform(-8, 8)))), white=float(f32(np.exp2(rng.uniform(-4, 19)))),
             adapt_brighter=float(f32(rng.uniform(0.01, 1.0))), adapt_darker=float(f32(rng.uniform(0.01, 1.0))))
    for k in ("weight_fovea", "weight_middle", "weight_periphery", "weight_uniform"):
        d[k] = int(rng.choice([0, 1, 255, int(rng.integers(0, 256))]))
    return d


@pytest.mark.parametrize("seed", range(int(os.environ.get("FOVPT_FUZZEX_TO", "8"))))
def test_seeded_sweep(oracle, seed):
    rng = np.random.default_rng(1000 + seed)
    w, h = int(rng.integers(1, 97)), int(rng.integers(1, 97))
    uniform = rng.random() < 0.25
    ri = int(rng.integers(0, 12))
    cfg = cfg_uniform(1) if uniform else cfg_foveated(ri, ri + int(rng.integers(0, 24)), (1, 1, 1))
    gaze = (int(rng.integers(-8, w + 8)) & 0xffffffff, int(rng.integers(-8, h + 8)) & 0xffffffff)
    r = _cornell((w, h), cfg, gaze=gaze)
    r.render()
    ck = Checker(oracle, r)
    for k in range(3):
        img = np.exp2(rng.uniform(-20, 20, (h, w, 4))).astype(np.float32) * f32(np.exp2(rng.uniform(-6, 6)))
        odd = rng.random((h, w))
        for v, p in ((0.0, 0.05), (np.nan, 0.02), (np.inf, 0.02), (-2.0, 0.02), (DENORMAL, 0.02)):
            img[odd < p] = v
            odd[odd < p] = 1.0
            odd -= p
        ck.step(_random_config(rng), img.astype(np.float32), label=(seed, k))
    r.close()


# ---- 11. the C++ drop-in --------------------------------------------------------------------------------------------------------------
def test_cpp_dropin_expose(tmp_path):
    """SampleRenderer::exposePost() / expose() / exposeState() of include/SimplePathtracer.h: the same pixels and states as Python."""
    exe, out = build_dropin(tmp_path, "expose_gpu_test"), str(tmp_path / "expose_out.bin")
    run_dropin(exe, out)
    n = 160 * 96
    raw = np.fromfile(out, np.uint32)
    px = raw[:3 * n].reshape(3, 96, 160)
    states = raw[3 * n:].tobytes()
    assert len(states) == 64
    r = dropin_renderer(write_guides=True)
    c, _ = ecfg(dict(adapt_brighter=0.5, adapt_darker=0.5))
    for k in range(2):
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = 80 + 40 * k, 48 - 30 * k
        r.render()
        r.post()
        r.expose(c, r.post_buffers()[0])
        assert np.array_equal(px[k], r.downloadExposedPixels()), k
        assert states[32 * k:32 * k + 32] == bytes(r.expose_state()), k
    st = r.expose_state()
    assert st.steps == 2 and st.ev != st.ev_metered and len(np.unique(px[1])) > 20
    c, _ = ecfg(dict(mode=abi.EXPOSE_FIXED, tone=abi.TONE_ACES, exposure=0.75, adapt_brighter=0.5, adapt_darker=0.5))
    r.expose(c)
    assert np.array_equal(px[2], r.downloadExposedPixels())
    r.close()
