"""fovpt_resize and the post-frame stages, all of them on one context: a context that has run every stage with its own outputs at
48 x 32, at 80 x 56 and at 24 x 16 gives at 24 x 16, bit for bit, what a fresh context gives there; after a resize and before a
render every stage is refused with FOVPT_E_NO_FRAME while the expose, focus and quality records stay; and a resize makes no buffer
that no stage has made.  The scene is the Cornell box; nothing here is compared with a restatement (each stage's own test does that)."""
import ctypes as C

import numpy as np
import pytest

from fovpathtracing_optixcodelatest_amd import abi, lib, renderer, scenes

from common import cfg_foveated, make_gpu

pytestmark = pytest.mark.gpu
E_INVALID, E_NO_FRAME = -1, -5
SIZES = [(48, 32), (80, 56), (24, 16)]
CAMERA = scenes.CORNELL_CAMERA
PROBE = scenes.sky_probe()
# the camera the warp and the lens aim at: the frame's, a little to the side and turned
TO = dict(eye=(300.0, 280.0, -790.0), lookat=(260.0, 265.0, 0.0), up=CAMERA["up"], fovy=CAMERA["fovy"])


def config():
    c = cfg_foveated(4, 8, (1, 2, 4))
    c.write_guides = 1
    return c


def camera(d, size):
    return renderer.Camera(d["eye"], d["lookat"], d["up"], d["fovy"], size[0] / float(size[1]))


def to_size(r, size):
    """The context at `size`, resized where it is of another, with the camera and gaze of that size; nothing rendered."""
    f = r.launchParams.frame
    if (f.size.x, f.size.y) != size:
        r.resize(size)
    r.setCamera(camera(CAMERA, size))
    f.c.x, f.c.y = size[0] // 2, size[1] // 2


def reference_image(size):
    return np.random.default_rng(size[0]).integers(0, 1 << 32, (size[1], size[0]), dtype=np.uint64).astype(np.uint32)


def stage_calls(r, size, out_map=None, out_coc=None):
    """name -> the call of one stage into the context's own outputs, in the order drive() makes them."""
    def mode(defaults, fixed):
        c = defaults()
        if fixed is not None:
            c.mode = fixed
        return c

    return [
        ("denoise", lambda: r.denoise()),
        ("reconstruct", lambda: r.reconstruct()),
        ("temporal", lambda: r.temporal()),
        ("temporal_motion", lambda: r.temporal_motion(out_motion=r.motion_buffer())),
        ("post", lambda: r.post()),
        ("expose_fixed", lambda: r.expose(mode(r.expose_defaults, abi.EXPOSE_FIXED))),
        ("expose_auto", lambda: (r.expose_reset(), r.expose(mode(r.expose_defaults, abi.EXPOSE_AUTO)))),
        ("warp", lambda: r.warp(camera(TO, size), out_map=out_map)),
        ("focus_fixed", lambda: r.focus(mode(r.focus_defaults, abi.FOCUS_FIXED))),
        ("focus_auto", lambda: (r.focus_reset(), r.focus(mode(r.focus_defaults, abi.FOCUS_AUTO), out_coc=out_coc))),
        ("lens", lambda: r.lens(None, camera(TO, size))),
        ("quality", lambda: r.qualityAsync(reference_image(size))),
    ]


def drive(r, size):
    """One render at `size` and every stage once (expose and focus FIXED, then AUTO after their reset) -> name -> bytes of
    everything the stages left: the own colour and rgba8 of each, the records, the map, the radii, the history, the motion."""
    import torch
    to_size(r, size)
    r.launchParams.frame.subframe_index = 0
    r.render()
    w, h = size
    out_map = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    out_coc = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    pair = lambda p: (p[0].tobytes(), p[1].tobytes())
    own = dict(
        denoise=lambda: (r.downloadDenoisedColor().tobytes(), r.downloadDenoisedPixels().tobytes()),
        reconstruct=lambda: (r.downloadReconstructedColor().tobytes(), r.downloadReconstructedPixels().tobytes()),
        temporal=lambda: (r.downloadTemporalColor().tobytes(), r.downloadTemporalPixels().tobytes(), r.downloadTemporalHistory().tobytes()),
        temporal_motion=lambda: (r.downloadTemporalColor().tobytes(), r.downloadTemporalPixels().tobytes(), r.downloadTemporalHistory().tobytes(),
                                 r.downloadMotion().tobytes()),
        post=lambda: (r.downloadPostColor().tobytes(), r.downloadPostPixels().tobytes(), r.downloadTemporalHistory().tobytes()),
        expose_fixed=lambda: (r.downloadExposedColor().tobytes(), r.downloadExposedPixels().tobytes()),
        expose_auto=lambda: (r.downloadExposedColor().tobytes(), r.downloadExposedPixels().tobytes(), bytes(r.expose_state())),
        warp=lambda: (r.downloadWarpedColor().tobytes(), r.downloadWarpedPixels().tobytes(), bytes(r.warp_counts()), out_map.cpu().numpy().tobytes()),
        focus_fixed=lambda: pair(r.downloadFocus()),
        focus_auto=lambda: pair(r.downloadFocus()) + (bytes(r.focus_state()), out_coc.cpu().numpy().tobytes()),
        lens=lambda: pair(r.downloadLens()),
        quality=lambda: (bytes(r.readQuality(sums=True)),),
    )
    got = {}
    for name, call in stage_calls(r, size, out_map.data_ptr(), out_coc.data_ptr()):
        call()
        got[name] = own[name]()
    got["accum"] = (r.downloadAccum().tobytes(), r.downloadPixels().tobytes())
    return got


def debug_buffer_code(r, name):
    p, n = C.c_void_p(), C.c_size_t()
    return r._L.fovpt_debug_buffer(r._ctx, name, C.byref(p), C.byref(n))


@pytest.fixture(scope="module")
def contexts():
    """A: every stage at the three sizes in turn; B: only at the last.  -> (A, what A left at the last size, what B left there)"""
    a = make_gpu(scenes.cornell_box(), PROBE, CAMERA, SIZES[0], config())
    for size in SIZES:
        got_a = drive(a, size)
    b = make_gpu(scenes.cornell_box(), PROBE, CAMERA, SIZES[-1], config())
    got_b = drive(b, SIZES[-1])
    b.close()
    yield a, got_a, got_b
    a.close()


def test_resized_context_equals_a_fresh_one(contexts):
    a, got_a, got_b = contexts
    assert list(got_a) == list(got_b) and len(got_a) == 13
    for name in got_a:
        assert len(got_a[name]) == len(got_b[name]), name
        for k, (x, y) in enumerate(zip(got_a[name], got_b[name])):
            assert len(x) > 0 and x == y, (name, k)
    # the comparison is not of empty frames or of copies of one image
    n = SIZES[-1][0] * SIZES[-1][1]
    for name in ("denoise", "reconstruct", "temporal", "post", "expose_auto", "warp", "focus_auto", "lens"):
        assert len(got_a[name][0]) == 16 * n and len(got_a[name][1]) == 4 * n, name
        assert len(np.unique(np.frombuffer(got_a[name][1], np.uint32))) > 8, name
    assert got_a["expose_fixed"][1] != got_a["expose_auto"][1] and got_a["lens"][1] != got_a["warp"][1]
    assert abi.ExposeState.from_buffer_copy(got_a["expose_auto"][2]).steps == 1
    assert abi.FocusState.from_buffer_copy(got_a["focus_auto"][2]).steps == 1


def test_after_a_resize_and_before_a_render(contexts):
    """(runs after the comparison above: it resizes A)"""
    a, got_a, _ = contexts
    size = (40, 24)
    a.temporal_gbuffer()                                     # (the last step's, while there is one)
    to_size(a, size)
    # the records stay
    assert bytes(a.expose_state()) == got_a["expose_auto"][2] and bytes(a.focus_state()) == got_a["focus_auto"][2]
    assert bytes(a.readQuality(sums=True)) == got_a["quality"][0]
    with pytest.raises(lib.FovptError) as e:
        a.temporal_gbuffer()
    assert e.value.code == E_NO_FRAME
    for name, call in stage_calls(a, size):                  # (the AUTO calls reset their record first: the last thing that looks at it)
        with pytest.raises(lib.FovptError) as e:
            call()
        assert e.value.code == E_NO_FRAME, name
    assert bytes(a.readQuality(sums=True)) == got_a["quality"][0]
    drive(a, size)                                           # and the context goes on working
    assert a.expose_state().steps == 1 and a.focus_state().steps == 1 and a.temporal_gbuffer().width == size[0]


def test_a_resize_makes_no_buffer():
    names = (b"post_color", b"warp_keys", b"focus_scratch", b"expose_state")
    r = make_gpu(scenes.cornell_box(), PROBE, CAMERA, SIZES[0], config())
    r.render()
    r.lens()
    for size in (SIZES[1], SIZES[2]):
        to_size(r, size)
        for name in names:
            assert debug_buffer_code(r, name) == E_INVALID, (size, name)
    r.render()
    r.lens()
    assert all(r.lens_buffers())
    for name in names:
        assert debug_buffer_code(r, name) == E_INVALID, name
    r.close()
