"""fovpt_focus on the GPU against tests/focus_ref.py, bit for bit: both modes with every blur cap, two strengths and five gazes on
the box scene, synthetic G-buffers at the smallest sizes, an AUTO sequence with the reset paths, the caller's G-buffer
(fovpt_temporal_gbuffer) against the call's own trace, a FOV_OFF frame, the atrium, ordering with frames in flight, every rejection,
reallocation, and the C++ drop-in.  The restatement is fed the GPU's own G-buffer and colour; the conditions that keep a case from
being vacuous are asserted on the restatement's output."""
import ctypes as C

import numpy as np
import pytest

import focus_ref as fr
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer, scenes

from common import cfg_foveated, cfg_uniform, make_gpu
from gpu_common import (BOX_CAMERA, bits, box_renderer, build_dropin, debug_buffer, device_images, dropin_renderer, host_view,
                        run_dropin, upload, with_entries)

pytestmark = pytest.mark.gpu
E_INVALID, E_NO_SCENE, E_NO_FRAME = -1, -3, -5
SIZE = (193, 109)                                   # odd, and no multiple of the gather's 32 x 16 tile: partial edge tiles
PROBE = scenes.ambient_probe(64, 32, 2.5)
# the box scene seen from BOX_CAMERA (rows run upwards): the box around the centre, the slab above and beside it, sky below
GAZES = dict(box=(96, 54), floor=(40, 20), sky=(96, 95), corner=(2, 2), outside=(300, 50))
f32 = np.float32


def fcfg(d=None):
    """fovpt_focus_defaults with the entries of d replaced -> (abi.FocusConfig, the dict the restatement takes)."""
    c = with_entries(renderer.SampleRenderer.focus_defaults(), d)
    return c, c.as_dict()


def state_tuple(s):
    """A state record, ctypes or the restatement's, as comparable integers (floats by their bits)."""
    get = (lambda k: getattr(s, k)) if isinstance(s, abi.FocusState) else (lambda k: s[k])
    return tuple(int(np.float32(get(k)).view(np.uint32)) for k in ("focus_metered", "inv_focus", "focus")) + (int(get("count")), int(get("steps")))


def gaze_of(r):
    f = r.launchParams.frame
    return (f.c.x, f.c.y)


class Checker:
    """Follows a renderer's focus state with the restatement: step() runs one fovpt_focus into caller's buffers and compares every
    output and the state record."""

    def __init__(self, oracle, r):
        self.oracle, self.r, self.state = oracle, r, fr.new_state()

    def reset(self):
        self.state = fr.new_state()

    def step(self, d, gb, color, gbuffer=None, in_ptr=None, label=None):
        f = self.r.launchParams.frame
        size = (f.size.x, f.size.y)
        cfg, full = fcfg(d)
        oc, op, oz = device_images(size, 16, 4, 4)
        self.r.focus(cfg, gbuffer, in_ptr, oc.data_ptr(), op.data_ptr(), oz.data_ptr())
        want = fr.focus(self.oracle, gb, gaze_of(self.r), color, full, self.state)
        self.state = want["state"]
        got = self.r.focus_state()
        print(label, "state", state_tuple(got), "sharp", int((want["covering"] == 1).sum()), "cap", int((want["coc"] == full["max_radius"]).sum()),
              "acted", int(want["acted"].sum()))
        assert state_tuple(got) == state_tuple(self.state), (label, state_tuple(got), state_tuple(self.state))
        assert np.array_equal(bits(host_view(oz, "coc")), bits(want["coc"])), label
        assert np.array_equal(bits(host_view(oc, "color")), bits(want["color"])), label
        assert np.array_equal(host_view(op, "rgba"), want["rgba"]), label
        return want


# ---- 1. bit for bit ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def box():
    r = box_renderer(SIZE, cfg_foveated(12, 36, (1, 1, 2)), write_guides=True)
    yield r
    r.close()


@pytest.mark.parametrize("where", list(GAZES))
def test_bit_for_bit(oracle, box, where):
    r = box
    r.launchParams.frame.c.x, r.launchParams.frame.c.y = GAZES[where]
    r.render()
    gb, color = r.downloadGBuffer(), r.downloadAccum()
    r.focus_reset()
    ck = Checker(oracle, r)
    for mode in (abi.FOCUS_FIXED, abi.FOCUS_AUTO):
        for max_radius in (0, 1, 3, 8):
            for strength in (40.0, 400.0):
                d = dict(mode=mode, max_radius=max_radius, strength=strength, focus_distance=6.5, focus_default=7.0, meter_radius=12)
                want = ck.step(d, gb, color, label=(where, mode, max_radius, strength))
                if max_radius == 0:
                    assert np.array_equal(bits(want["color"]), bits(color))
                if (max_radius, strength) == (3, 40.0):                # what keeps the case from being vacuous
                    coc = want["coc"]
                    assert (want["covering"] == 1).sum() > 100 and (coc == 3).sum() > 100 and ((coc > 0.5) & (coc < 3)).sum() > 100
                    assert want["acted"].sum() > 100 and want["cut"].any()
        if mode == abi.FOCUS_FIXED:
            assert r.focus_state().steps == 0                          # FIXED leaves the state alone (none was made yet, or a reset one)
    st = r.focus_state()
    assert st.steps == 8
    assert (st.count > 0) == (where in ("box", "floor", "corner")), (where, st.count)
    if where == "corner":
        assert 0 < st.count < 441                                      # the disc is cut by the frame's edge
    if where in ("sky", "outside"):
        assert st.focus_metered == f32(1.0) / (f32(1.0) / f32(7.0)) or st.focus_metered == f32(7.0)      # the present focus: focus_default's
    # the frame and its G-buffer are as they were
    assert np.array_equal(bits(r.downloadAccum()), bits(color))


def test_into_the_renderers_own_buffers(oracle, box):
    r = box
    r.launchParams.frame.c.x, r.launchParams.frame.c.y = GAZES["box"]
    r.render()
    gb, color = r.downloadGBuffer(), r.downloadAccum()
    r.focus_reset()
    r.focus()                                                          # the defaults
    got_c, got_p = r.downloadFocus()
    want = fr.focus(oracle, gb, gaze_of(r), color, fr.DEFAULTS, fr.new_state())
    assert np.array_equal(bits(got_c), bits(want["color"])) and np.array_equal(got_p, want["rgba"])
    assert state_tuple(r.focus_state()) == state_tuple(want["state"]) and want["state"]["count"] == 441
    assert debug_buffer(r, "focus_state")[1] == 32 and debug_buffer(r, "focus_scratch")[1] >= SIZE[0] * SIZE[1] * 8
    pairs = r.download(debug_buffer(r, "focus_scratch")[0], np.empty((SIZE[1], SIZE[0], 2), np.float32))
    assert np.array_equal(bits(pairs[..., 0]), bits(want["coc"])) and np.array_equal(bits(pairs[..., 1]), bits(want["tp"]))


# ---- 2. synthetic G-buffers ----------------------------------------------------------------------------------------------------------
def synthetic(size, seed):
    w, h = size
    rng = np.random.default_rng(seed)
    prim = rng.integers(0, 1000, (h, w)).astype(np.uint32)
    prim[rng.random((h, w)) < 1 / 3] = fr.MISS
    pos = rng.uniform(-5, 5, (h, w, 4)).astype(np.float32)
    pos[..., 3] = np.exp2(rng.uniform(-3, 3, (h, w))).astype(np.float32)      # six octaves: a depth discontinuity at every pixel
    pos[prim == fr.MISS, 3] = -1.0
    color = rng.uniform(0, 8, (h, w, 4)).astype(np.float32)
    return dict(prim=prim, position=pos), color


@pytest.mark.parametrize("size", [(1, 1), (17, 17), (70, 9), (9, 70), (37, 23)], ids=lambda s: "%dx%d" % s)
def test_synthetic_gbuffers(oracle, size):
    r = box_renderer(size, cfg_uniform(1), (size[0] // 2, size[1] // 2), write_guides=True)
    r.render()
    ck = Checker(oracle, r)
    for seed, d in enumerate((dict(strength=3.0, max_radius=8), dict(strength=0.7, max_radius=5, rank_permille=900, meter_radius=64),
                              dict(strength=9.0, max_radius=2, mode=abi.FOCUS_FIXED, focus_distance=0.5),
                              dict(strength=float(np.nextafter(f32(0.5), f32(0))), max_radius=3, mode=abi.FOCUS_FIXED))):
        gb, color = synthetic(size, seed)
        dp, dq, dc = upload(gb["prim"]), upload(gb["position"]), upload(color)
        g = abi.GBufferPtrs()
        g.prim, g.position, g.width, g.height = dp.data_ptr(), dq.data_ptr(), size[0], size[1]
        want = ck.step(d, gb, color, g, dc.data_ptr(), label=(size, seed))
        if size != (1, 1):
            assert (want["covering"] > 1).any() and want["cut"].any(), (size, seed)
            if seed < 2:
                assert want["acted"].any(), (size, seed)
    r.close()


# ---- 3. an AUTO sequence and the reset paths ---------------------------------------------------------------------------------------
def test_an_auto_sequence_and_the_reset_paths(oracle):
    r = box_renderer(SIZE, cfg_foveated(12, 36, (1, 1, 2)), write_guides=True)
    ck = Checker(oracle, r)
    rates = [(1.0, 1.0), (0.5, 0.25), (0.125, 0.75), (0.3, 0.7), (0.9, 0.05)]
    seen, gazes = [], dict(GAZES, far=(170, 45))                      # far: the slab behind the box
    for k, (where, (nearer, farther)) in enumerate(zip(("box", "far", "sky", "box", "corner"), rates)):
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = gazes[where]
        r.launchParams.frame.subframe_index = k
        r.render()
        ck.step(dict(adapt_nearer=nearer, adapt_farther=farther, strength=40.0, max_radius=4, rank_permille=100 + 200 * k), r.downloadGBuffer(),
                r.downloadAccum(), label=(k, where))
        seen.append(r.focus_state().focus)
    st = r.focus_state()
    # farther, nothing to meter (the focus stays), nearer, and each by its own rate: no step but the first lands on its target
    assert st.steps == 5 and seen[1] > seen[0] and seen[2] == seen[1] and seen[3] < seen[2] and st.focus != st.focus_metered
    r.focus_reset()
    ck.reset()
    assert r.focus_state().steps == 0
    gb, color = r.downloadGBuffer(), r.downloadAccum()
    ck.step(dict(adapt_nearer=0.5, adapt_farther=0.5), gb, color, label="after reset")
    st = r.focus_state()
    assert st.steps == 1 and st.inv_focus == f32(1.0) / f32(st.focus_metered)
    # the state survives fovpt_resize and fovpt_set_probe
    r.resize((40, 24))
    r.setCamera(r.lastSetCamera)
    r.launchParams.frame.c.x, r.launchParams.frame.c.y = 5, 5
    with pytest.raises(lib.FovptError) as e:                 # (nothing rendered at this size yet)
        r.focus()
    assert e.value.code == E_NO_FRAME
    r.render()
    ck.step(dict(adapt_nearer=0.5, adapt_farther=0.5), r.downloadGBuffer(), r.downloadAccum(), label="after resize")
    st = r.focus_state()
    assert st.steps == 2 and st.count > 0
    r.setProbe(renderer.ProbeData(scenes.ambient_probe(32, 16, 1.0)).BuildCDF())
    assert r.focus_state().steps == 2
    # fovpt_set_scene resets it
    from test_temporal_gpu import _scene_again
    _scene_again(r)
    assert r.focus_state().steps == 0
    ck.reset()
    r.render()
    ck.step(dict(adapt_nearer=0.5, adapt_farther=0.5), r.downloadGBuffer(), r.downloadAccum(), label="after set_scene")
    assert r.focus_state().steps == 1
    r.close()


# ---- 4. the caller's G-buffer --------------------------------------------------------------------------------------------------------
def test_the_temporal_steps_gbuffer_saves_the_trace(oracle):
    r = box_renderer(SIZE, cfg_foveated(12, 36, (1, 1, 2)), write_guides=True)
    r.render()
    r.post()
    g = r.temporal_gbuffer()
    cfg, full = fcfg(dict(strength=40.0))
    post_color = r.post_buffers()[0]
    r.focus(cfg, None, post_color)                           # its own trace: into fovpt_gbuffer's buffers
    own = r.downloadFocus() + (state_tuple(r.focus_state()),)
    # fovpt_gbuffer's buffers now hold another view's G-buffer: the call with the step's set must not touch them
    r.setCamera(renderer.Camera((4.0, 3.0, 6.0), (1.2, 0.5, -1.0), BOX_CAMERA["up"], BOX_CAMERA["fovy"], SIZE[0] / float(SIZE[1])))
    other = r.gbuffer()
    r.setCamera(renderer.Camera(BOX_CAMERA["eye"], BOX_CAMERA["lookat"], BOX_CAMERA["up"], BOX_CAMERA["fovy"], SIZE[0] / float(SIZE[1])))
    assert other.prim != g.prim and other.position != g.position
    before = r.downloadGBuffer(other)
    r.focus_reset()
    oc, op, oz = device_images(SIZE, 16, 4, 4)
    r.focus(cfg, g, post_color, oc.data_ptr(), op.data_ptr(), oz.data_ptr())
    assert np.array_equal(bits(host_view(oc, "color")), bits(own[0])) and np.array_equal(host_view(op, "rgba"), own[1])
    assert state_tuple(r.focus_state()) == own[2]
    after = r.downloadGBuffer(other)
    for k in before:
        assert np.array_equal(bits(before[k]), bits(after[k])), k
    assert (before["prim"] != r.downloadGBuffer(g)["prim"]).mean() > 0.05      # (the two sets do hold different views)
    # against the restatement on the step's set
    want = fr.focus(oracle, r.downloadGBuffer(g), gaze_of(r), r.downloadPostColor(), full, fr.new_state())
    assert np.array_equal(bits(own[0]), bits(want["color"])) and np.array_equal(bits(host_view(oz, "coc")), bits(want["coc"]))
    assert (want["covering"] > 1).any() and (want["covering"] == 1).any()
    r.close()


# ---- 5. a FOV_OFF frame and the atrium -----------------------------------------------------------------------------------------------
def test_fov_off_160x90(oracle):
    size = (160, 90)
    r = box_renderer(size, cfg_uniform(2), (80, 45), write_guides=True)
    r.render()
    ck = Checker(oracle, r)
    gb, color = r.downloadGBuffer(), r.downloadAccum()
    for d in (dict(strength=40.0), dict(strength=100.0, max_radius=8, mode=abi.FOCUS_FIXED, focus_distance=9.0)):
        want = ck.step(d, gb, color, label=d)
        assert (want["covering"] > 1).any() and want["acted"].any()
    r.close()


def test_the_atrium(oracle):
    """A scene with depth complexity: columns in front of walls."""
    r = make_gpu(scenes.atrium(8000), PROBE, scenes.ATRIUM_CAMERA, SIZE, cfg_foveated(12, 36, (1, 1, 2)))
    r.render()
    ck = Checker(oracle, r)
    gb, color = r.downloadGBuffer(), r.downloadAccum()
    t = gb["position"][..., 3][gb["prim"] != fr.MISS]
    scale = float(np.median(t))                                        # the scene's own distances set the strength
    want = ck.step(dict(strength=6.0 * scale, max_radius=8, meter_radius=20), gb, color, label="atrium")
    coc = want["coc"]
    assert want["state"]["count"] > 0 and (want["covering"] == 1).any() and (coc == 8).any() and ((coc > 0.5) & (coc < 8)).sum() > 100
    assert want["acted"].sum() > 100
    r.close()


# ---- 6. ordering ---------------------------------------------------------------------------------------------------------------------
def test_focus_is_ordered_with_frames_in_flight():
    """render_async, focus, render_async, focus with no synchronisation in between: what the same sequence gives with a synchronise
    after every call."""
    import torch
    size = (384, 216)
    cfg = cfg_foveated(20, 60, (4, 8, 16))
    cfg.frames_in_flight = 2
    r = box_renderer(size, cfg, write_guides=True)
    fc, _ = fcfg(dict(strength=40.0, adapt_nearer=0.5, adapt_farther=0.25))
    views = [((190, 108), 0), ((300, 40), 1), ((80, 60), 2)]
    outs = [[device_images(size, 16, 4, 4) for _ in views] for _ in range(2)]
    states = []
    for sync, out in zip((True, False), outs):
        for g, k in views:                                   # the accum buffer's leftovers where no pass writes, as all views leave them
            r.launchParams.frame.c.x, r.launchParams.frame.c.y = g
            r.launchParams.frame.subframe_index = k
            r.render()
        r.focus_reset()
        for (g, k), (oc, op, oz) in zip(views, out):
            r.launchParams.frame.c.x, r.launchParams.frame.c.y = g
            r.launchParams.frame.subframe_index = k
            r.render_async()
            if sync:
                r.synchronize()
            r.focus(fc, None, None, oc.data_ptr(), op.data_ptr(), oz.data_ptr())
            if sync:
                r.synchronize()
        r.synchronize()
        states.append(state_tuple(r.focus_state()))
    for want, got in zip(*outs):
        for x, y in zip(want, got):
            assert torch.equal(x, y)
    assert states[0] == states[1] and states[0][4] == 3
    a, b = host_view(outs[0][0][1], "rgba"), host_view(outs[0][2][1], "rgba")
    assert (a != b).mean() > 0.1                             # (the frames differ: the comparison is not of copies)
    r.close()


# ---- 7. rejections -------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_everything_unchanged():
    r = box_renderer(SIZE, cfg_foveated(12, 36, (1, 1, 2)), write_guides=True)
    L = lib.load()
    with pytest.raises(lib.FovptError) as e:                 # nothing rendered yet
        r.focus()
    assert e.value.code == E_NO_FRAME and r.focus_state().steps == 0
    r.render()
    oc, op, oz = device_images(SIZE, 16, 4, 4)
    good, _ = fcfg(dict(strength=40.0))
    r.focus(good, None, None, oc.data_ptr(), op.data_ptr(), oz.data_ptr())
    r.focus(good)
    g = r.gbuffer()
    r.synchronize()
    scratch = debug_buffer(r, "focus_scratch")[0]

    def everything():
        own = r.downloadFocus()
        return (bytes(r.focus_state()), own[0].tobytes(), own[1].tobytes(), oc.cpu().numpy().tobytes(), op.cpu().numpy().tobytes(),
                oz.cpu().numpy().tobytes(), r.download(scratch, np.empty((SIZE[1], SIZE[0], 2), np.float32)).tobytes())

    before = everything()
    outs = dict(out_color=oc.data_ptr(), out_rgba=op.data_ptr(), out_coc=oz.data_ptr())

    def refuse(code, label, **kw):
        args = dict(cfg=good, gbuffer=None, in_color=None, **outs)
        args.update(kw)
        with pytest.raises(lib.FovptError) as e:
            r.focus(**args)
        assert e.value.code == code, label
        assert everything() == before, label

    nan, inf = float("nan"), float("inf")
    bad_values = dict(mode=(-1, 2, 7), meter_radius=(-1, 65, 1 << 20), rank_permille=(-1, 1001), max_radius=(-1, 9, 1 << 20),
                      strength=(nan, -1.0, -1e-30, 1.1e6, inf), focus_distance=(nan, 0.0, -1.0, 0.9e-6, 1.1e6, inf),
                      focus_default=(nan, 0.0, -1.0, 0.9e-6, 1.1e6, inf), adapt_nearer=(nan, 0.0, -0.5, 1.0001, inf),
                      adapt_farther=(nan, 0.0, -0.5, 1.0001, inf))
    for k, values in bad_values.items():
        for v in values:
            refuse(E_INVALID, (k, v), cfg=fcfg({k: v})[0])
    for i in range(7):
        c = fcfg()[0]
        c._reserved[i] = 1
        refuse(E_INVALID, ("_reserved", i), cfg=c)
    # null arguments
    lp = C.byref(r.launchParams)
    assert L.fovpt_focus(r._ctx, None, C.byref(good), None, None, None, None, None) == E_INVALID
    assert L.fovpt_focus(r._ctx, lp, None, None, None, None, None, None) == E_INVALID
    col_, rgba_ = C.c_void_p(), C.c_void_p()
    assert L.fovpt_focus_buffers(r._ctx, None, C.byref(rgba_)) == E_INVALID and L.fovpt_focus_buffers(r._ctx, C.byref(col_), None) == E_INVALID
    assert L.fovpt_focus_state(r._ctx, None) == E_INVALID
    assert everything() == before
    # the G-buffer
    for k, v in (("width", SIZE[0] - 1), ("height", SIZE[1] + 1), ("prim", None), ("position", None)):
        bad = abi.GBufferPtrs.from_buffer_copy(bytes(g))
        setattr(bad, k, v)
        refuse(E_INVALID, ("gbuffer", k), gbuffer=bad)
    # a null input
    f = r.launchParams.frame
    keep = f.accum_buffer
    f.accum_buffer = None
    refuse(E_INVALID, "null accum_buffer")
    f.accum_buffer = keep
    # aliasing: an output that is an input or another output
    fc_, fp_ = r.focus_buffers()
    refuse(E_INVALID, "out_color is in_color", in_color=oc.data_ptr())
    refuse(E_INVALID, "out_color is accum", out_color=keep)
    refuse(E_INVALID, "out_rgba is in_color", in_color=op.data_ptr())
    refuse(E_INVALID, "out_coc is in_color", in_color=oz.data_ptr())
    refuse(E_INVALID, "out_coc is out_rgba", out_coc=op.data_ptr())
    refuse(E_INVALID, "out_coc is out_color", out_coc=oc.data_ptr())
    refuse(E_INVALID, "out_rgba is out_color", out_rgba=oc.data_ptr())
    refuse(E_INVALID, "out_coc is the own colour", out_color=None, out_coc=fc_)
    refuse(E_INVALID, "out_coc is the own rgba", out_rgba=None, out_coc=fp_)
    refuse(E_INVALID, "out_coc is the G-buffer's prim", gbuffer=g, out_coc=g.prim)
    refuse(E_INVALID, "out_color is the G-buffer's position", gbuffer=g, out_color=g.position)
    refuse(E_INVALID, "out_color is the traced G-buffer's position", out_color=g.position)
    refuse(E_INVALID, "out_color is the scratch", out_color=scratch)
    # the frame: another size, then another scene, then a tile shard
    f.size.x -= 4
    with pytest.raises(lib.FovptError) as e:
        r.focus(good, **outs)
    f.size.x += 4                                            # (the downloads of everything() go by this size)
    assert e.value.code == E_NO_FRAME and everything() == before
    keep_trav = r.launchParams.traversable
    r.launchParams.traversable = keep_trav + 1               # not the current scene: only the traced G-buffer needs it
    refuse(E_NO_SCENE, "no scene")
    r.focus_reset()
    r.focus(good, g, None, **outs)
    r.focus_reset()
    r.focus(good, g)
    assert everything()[1:] == before[1:]                    # (the same call again, with a caller's G-buffer)
    r.launchParams.traversable = keep_trav
    before = everything()
    c = r.config
    c.world, c.rank = 2, 0
    r.config = c
    r.render()
    refuse(E_INVALID, "world 2")
    c.world, c.rank = 1, 0
    r.config = c
    r.render()
    r.focus(good, **outs)                                    # the valid call after them
    assert r.focus_state().steps == before_steps(before) + 1
    r.close()


def before_steps(everything):
    return abi.FocusState.from_buffer_copy(everything[0]).steps


# ---- 8. reallocation -----------------------------------------------------------------------------------------------------------------
def test_resize_reallocates_the_focus_buffers(oracle):
    small, large = (96, 64), (200, 120)
    r = box_renderer(small, cfg_foveated(12, 36, (1, 1, 2)), write_guides=True)
    with pytest.raises(lib.FovptError) as e:
        r.focus_buffers()
    assert e.value.code == E_NO_FRAME
    with pytest.raises(lib.FovptError):
        debug_buffer(r, "focus_scratch")
    r.render()
    r.focus()
    assert debug_buffer(r, "focus_scratch")[1] == small[0] * small[1] * 8
    r.resize(large)
    r.setCamera(r.lastSetCamera)
    r.launchParams.frame.c.x, r.launchParams.frame.c.y = 100, 60
    assert debug_buffer(r, "focus_scratch")[1] == large[0] * large[1] * 8      # reallocated by the resize
    with pytest.raises(lib.FovptError) as e:                 # nothing rendered at this size yet
        r.focus()
    assert e.value.code == E_NO_FRAME
    r.render()
    gb, color = r.downloadGBuffer(), r.downloadAccum()
    cfg, full = fcfg(dict(strength=40.0))
    state = dict(zip(("focus_metered", "inv_focus", "focus"), (f32(getattr(r.focus_state(), k)) for k in ("focus_metered", "inv_focus", "focus"))),
                 count=r.focus_state().count, steps=r.focus_state().steps)
    assert state["steps"] == 1
    want = fr.focus(oracle, gb, gaze_of(r), color, full, state)
    r.focus(cfg)
    got_c, got_p = r.downloadFocus()
    assert np.array_equal(bits(got_c), bits(want["color"])) and np.array_equal(got_p, want["rgba"])
    assert state_tuple(r.focus_state()) == state_tuple(want["state"])
    r.close()


# ---- 9. the C++ drop-in --------------------------------------------------------------------------------------------------------------
def test_cpp_dropin_focus(tmp_path):
    """SampleRenderer::focus() / focusPost() / focusState() of include/SimplePathtracer.h: the same pixels and state as Python."""
    exe, out = build_dropin(tmp_path, "focus_gpu_test"), str(tmp_path / "focus_out.bin")
    run_dropin(exe, out)
    size = (160, 96)
    n = size[0] * size[1]
    raw = np.fromfile(out, np.uint8)
    px = raw[:12 * n].view(np.uint32).reshape(3, size[1], size[0])
    col = raw[12 * n:60 * n].view(np.float32).reshape(3, size[1], size[0], 4)
    states = [abi.FocusState.from_buffer_copy(raw[60 * n + 32 * k:60 * n + 32 * (k + 1)].tobytes()) for k in range(2)]
    strength = raw[60 * n + 64:60 * n + 68].view(np.float32)[0]
    r = dropin_renderer(write_guides=True)
    r.render()
    r.post()
    fc, _ = fcfg(dict(strength=40.0))
    r.focus(fc, r.temporal_gbuffer(), r.post_buffers()[0])
    got_c, got_p = r.downloadFocus()
    assert np.array_equal(px[0], got_p) and np.array_equal(bits(col[0]), bits(got_c))
    assert state_tuple(states[0]) == state_tuple(r.focus_state()) and states[1].steps == 2
    assert strength == f32(r.focus_strength(0.4)) or abs(strength - r.focus_strength(0.4)) < 1e-3 * strength
    fc, _ = fcfg(dict(mode=abi.FOCUS_FIXED, focus_distance=9.0, max_radius=8, strength=float(strength)))
    r.focus(fc)
    got_c, got_p = r.downloadFocus()
    assert np.array_equal(px[2], got_p) and np.array_equal(bits(col[2]), bits(got_c))
    assert (px[2] != px[0]).mean() > 0.05 and len(np.unique(px[0])) > 20
    r.close()
