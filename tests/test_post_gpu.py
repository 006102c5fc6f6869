"""fovpt_post on the GPU: bit for bit the separate stage calls on a twin context (every stage mask, moving camera and gaze), bit
for bit tests/post_ref.py on the GPU's own inputs while meshes move, the modes and reset paths, mixing with the temporal entry
points, the buffers it must leave alone, ordering with frames in flight, every error code with nothing enqueued and no state
moved, and the C++ drop-in."""
import ctypes as C

import numpy as np
import pytest

import temporal_ref as tr
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer, scenes

from common import cfg_foveated, cfg_uniform, make_gpu
from post_common import D, M, R, T, PostChecker, pcfg, same, separate
from gpu_common import bits, build_dropin, debug_buffer, dropin_renderer, run_dropin
from temporal_common import tcfg
from test_refit_gpu import cornell_motions, jitter
from test_temporal_gpu import ALL_CAPS, _atrium, _scene_again, _view

pytestmark = pytest.mark.gpu
E_INVALID, E_NO_SCENE, E_NO_FRAME = -1, -3, -5
CORNELL = scenes.CORNELL_CAMERA
PROBE = scenes.ambient_probe(64, 32, 2.0)
ATRIUM_PROBE = scenes.ambient_probe(96, 54, 2.5)


def _cornell(size, cfg):
    cfg.write_guides = 1
    return make_gpu(scenes.cornell_box(), PROBE, CORNELL, size, cfg)


def _cornell_view(r, k, size):
    eye = (CORNELL["eye"][0] + 12.0 * k, CORNELL["eye"][1] + 6.0 * k, CORNELL["eye"][2] + 10.0 * k)
    r.setCamera(renderer.Camera(eye, CORNELL["lookat"], CORNELL["up"], CORNELL["fovy"], size[0] / float(size[1])))


def _gaze(k, size):
    """Moves every frame; frame 2 looks at the frame's first pixel (the M and F offsets wrap as uint32), frame 5 at its last
    (blocks clamped onto the last row and column)."""
    return {2: (0, 0), 5: (size[0] - 1, size[1] - 1)}.get(k, (size[0] // 2 + 7 * k - 20, size[1] // 2 + 3 * k - 9))


# ---- 1. equals the separate calls ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stages, caps", [(R | T, None), (R | T | M, None), (R | T | M, ALL_CAPS), (D | R | T | M, None), (T | M, None), (R, None),
                                          (D, None)], ids=["RT", "RTM", "RTM_all_caps", "DRTM", "TM", "R", "D"])
def test_post_is_the_separate_calls(stages, caps):
    size = (193, 109)
    a, b = (_atrium(size, cfg_foveated(15, 48, (1, 2, 8))) for _ in range(2))
    pc = pcfg(stages, temporal=caps)
    for k in range(6):
        for r in (a, b):
            _view(r, k, size)
            r.launchParams.frame.c.x, r.launchParams.frame.c.y = _gaze(k, size)
            r.render()
        separate(a, pc, out_motion=a.motion_buffer() if stages & M else None)
        b.post(pc, out_motion=b.motion_buffer() if stages & M else None)
        same(a, b, stages, k)
    if stages & T:
        assert (b.downloadTemporalHistory()[..., 3] > 1).mean() > 0.5
    if stages & R:                                          # (the reconstruction did change pixels: the comparison is not of copies)
        assert (bits(b.downloadPostColor()) != bits(b.downloadAccum())).any(axis=-1).mean() > 0.1
    a.close()
    b.close()


# ---- 2. equals the restatement directly, while meshes move --------------------------------------------------------------------------
def test_post_matches_the_restatement_under_motion(oracle):
    size = (192, 120)
    r = _cornell(size, cfg_foveated(12, 36, (1, 2, 4)))
    ck = PostChecker(oracle, r, R | T | M, dict(temporal=ALL_CAPS))
    base = r.model
    (_, rigid), (_, scale), (_, point) = cornell_motions(base)
    tall, wall = base.meshes[4].vertex, base.meshes[2].vertex
    mesh = lambda gb: np.where(gb["prim"] == tr.MISS, -1, ck.mesh_of_prim[np.where(gb["prim"] == tr.MISS, 0, gb["prim"]).astype(np.int64)])

    def frame(k):
        _cornell_view(r, k, size)
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = size[0] // 2 + 9 * k - 20, size[1] // 2 + 4 * k - 8
        r.render()

    frame(0)
    ck.step()
    ck.update(rigid)                                          # host arrays, refit
    frame(1)
    o = ck.step(with_motion=False)                            # out_motion NULL
    cap = tr.caps(o["fill"], 0, ALL_CAPS)
    on_tall = (mesh(o["gb"]) == 4) & (cap > 1)
    assert on_tall.sum() > 100 and (o["history"][on_tall][:, 3] > 1).any()
    ck.update(scale, device=True)                             # device pointers, refit
    frame(2)
    ck.step()
    ck.update(point, rebuild=True)                            # FOVPT_UPDATE_REBUILD: the wall collapses to a point
    frame(3)
    ck.step()                                                 # one step after the rebuild
    ck.update({2: wall, 4: tall}, device=True)
    frame(4)
    o = ck.step()
    on_wall = (mesh(o["gb"]) == 2) & (tr.caps(o["fill"], 0, ALL_CAPS) > 1)   # the wall is back: its previous triangles have no area
    assert on_wall.sum() > 100 and (o["history"][on_wall][:, 3] == 1).all()
    assert (o["history"][..., 3] > 1).mean() > 0.3 and (o["motion"][..., 3] == 1).mean() > 0.5
    r.close()


# ---- 3. modes -----------------------------------------------------------------------------------------------------------------------
def test_a_fov_off_frame_is_the_plain_step(oracle):
    size = (160, 90)
    a, b = (_atrium(size, cfg_uniform(1)) for _ in range(2))
    ck = PostChecker(oracle, b, R | T | M, dict(temporal=ALL_CAPS))
    for k in range(3):
        for r in (a, b):
            _view(r, k, size)
            r.render()
        a.temporal_motion(tcfg(ALL_CAPS), None, None, None, a.motion_buffer())      # no reconstruction at all
        o = ck.step()
        assert np.array_equal(bits(a.downloadTemporalColor()), bits(o["color"])) and np.array_equal(a.downloadTemporalPixels(), b.downloadPostPixels())
        assert np.array_equal(bits(a.downloadTemporalHistory()), bits(o["history"])) and np.array_equal(bits(a.downloadMotion()), bits(o["motion"]))
    assert (o["history"][..., 3] > 1).mean() > 0.5
    a.close()
    b.close()


@pytest.mark.parametrize("mode", ["levels_1", "levels_2", "no_guides", "in_color", "caller_outputs"])
def test_post_modes(oracle, mode):
    import torch
    size = (160, 96)
    cfg = cfg_foveated(12, 36, (1, 2, 4))
    if mode == "no_guides":                                  # remodulate = 0 on a frame rendered with write_guides = 0
        r = make_gpu(scenes.atrium(8000), ATRIUM_PROBE, scenes.ATRIUM_CAMERA, size, cfg)
        assert r.config.write_guides == 0
    else:
        r = _atrium(size, cfg)
    rc = dict(levels_1=dict(levels=1), levels_2=dict(levels=2), no_guides=dict(remodulate=0)).get(mode)
    ck = PostChecker(oracle, r, R | T | M, dict(reconstruct=rc, temporal=ALL_CAPS))
    h, w = size[1], size[0]
    for k in range(3):
        _view(r, k, size)
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = _gaze(k, size)
        r.render()
        if mode == "in_color":
            inp = np.random.default_rng(k).uniform(0, 2, (h, w, 4)).astype(np.float32)
            dev = torch.from_numpy(inp).cuda()
            torch.cuda.synchronize()
            o = ck.step(inp, dev.data_ptr())
        elif mode == "caller_outputs":
            oc = torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda")
            op = torch.zeros((h, w), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            o = ck.step(out=(oc.data_ptr(), op.data_ptr()))
        else:
            o = ck.step()
    assert (o["history"][..., 3] > 1).mean() > 0.5
    if mode == "no_guides":
        with pytest.raises(lib.FovptError) as e:             # and remodulate = 1 needs them
            r.post()
        assert e.value.code == E_INVALID
    if mode == "caller_outputs":
        with pytest.raises(lib.FovptError) as e:             # the context's own post buffers were never needed
            debug_buffer(r, "post_color")
        assert e.value.code == E_INVALID
    r.close()


def test_post_reset_paths(oracle):
    """The first call, and the call after fovpt_temporal_reset, fovpt_resize and fovpt_set_scene: the reconstruction, n == 1."""
    size = (160, 96)
    r = _cornell(size, cfg_foveated(12, 36, (1, 2, 4)))
    ck = PostChecker(oracle, r, R | T | M, dict(temporal=ALL_CAPS))
    motions = cornell_motions(r.model)

    def fresh(label):
        r.render()
        o = ck.step()
        r.reconstruct()
        assert np.array_equal(bits(o["color"]), bits(r.downloadReconstructedColor())), label
        assert (o["history"][..., 3] == 1).all() and not o["motion"].any(), label

    def carried(k):
        ck.update(motions[k][1])
        r.render()
        assert (ck.step()["history"][..., 3] > 1).mean() > 0.5

    fresh("first")
    carried(0)
    r.temporal_reset()
    ck.reset()
    fresh("reset")
    carried(1)
    r.resize((144, 80))
    r.setCamera(renderer.Camera(CORNELL["eye"], CORNELL["lookat"], CORNELL["up"], CORNELL["fovy"], 144 / 80.0))
    ck.reset()
    fresh("resize")
    assert debug_buffer(r, "post_color")[1] >= 144 * 80 * 16
    carried(2)
    _scene_again(r)                                           # the model's own positions again, tracking off until the next step
    ck = PostChecker(oracle, r, R | T | M, dict(temporal=ALL_CAPS))
    fresh("set_scene")
    carried(0)
    r.close()


# ---- 4. mixing with the temporal entry points ---------------------------------------------------------------------------------------
def test_post_mixes_with_the_temporal_calls():
    size = (160, 96)
    a, b = (_cornell(size, cfg_foveated(12, 36, (1, 2, 4))) for _ in range(2))
    pc = pcfg(R | T | M, temporal=ALL_CAPS)
    d = tcfg(ALL_CAPS)
    motions = cornell_motions(a.model)
    for k, call in enumerate(("post", "temporal_motion", "post", "temporal", "post")):
        for r in (a, b):
            if k:
                r.update_vertices(motions[k % 2][1])
            _cornell_view(r, k, size)
            r.render()
        ma, mb = a.motion_buffer(), b.motion_buffer()
        if call == "post":
            separate(a, pc, out_motion=ma)
            b.post(pc, out_motion=mb)
            same(a, b, R | T | M, k)
        elif call == "temporal_motion":
            for r, m in ((a, ma), (b, mb)):
                r.temporal_motion(d, None, None, None, m)
        else:
            for r in (a, b):
                r.temporal(d)
        assert np.array_equal(bits(a.downloadTemporalHistory()), bits(b.downloadTemporalHistory())), (k, call)
        if k:
            assert (b.downloadTemporalHistory()[..., 3] > 1).mean() > 0.3, (k, call)
    a.close()
    b.close()


def test_an_update_before_tracking_starts_drops_the_history_once(oracle):
    """As test_temporal_motion_gpu.test_an_update_before_tracking_starts_drops_the_history expects of fovpt_temporal_motion."""
    size = (96, 64)
    r = _cornell(size, cfg_foveated(10, 24, (1, 2, 4)))
    ck = PostChecker(oracle, r, R | T | M, dict(temporal=ALL_CAPS))
    r.render()
    ck.step(stages=R | T)                                     # no MOTION: tracking stays off
    ck.update(cornell_motions(r.model)[0][1])                 # where the block was is not recorded
    r.render()
    o = ck.step()                                             # (the checker expects no history either)
    assert (o["history"][..., 3] == 1).all() and not o["motion"].any()
    r.render()
    assert (ck.step()["history"][..., 3] > 1).mean() > 0.5    # from here on it is carried, and updates are tracked
    ck.update(cornell_motions(r.model)[1][1])
    r.render()
    assert (ck.step()["history"][..., 3] > 1).mean() > 0.5
    r.close()


# ---- 5. buffers left alone ----------------------------------------------------------------------------------------------------------
def test_post_leaves_the_reconstruction_and_gbuffer_buffers_alone():
    size = (160, 96)
    r = _atrium(size, cfg_foveated(12, 36, (1, 2, 4)))
    with pytest.raises(lib.FovptError) as e:
        debug_buffer(r, "post_color")
    assert e.value.code == E_INVALID
    _view(r, 3, size)                                         # the sentinel frame: another camera
    r.render()
    r.reconstruct()
    g = r.gbuffer()
    h, w = size[1], size[0]

    def snapshot():
        col, rgba = r.reconstruct_buffers()
        out = [r.download(col, np.empty((h, w, 4), np.float32)), r.download(rgba, np.empty((h, w), np.uint32)),
               r.download(g.prim, np.empty((h, w), np.uint32))]
        return out + [r.download(getattr(g, k), np.empty((h, w, 4), np.float32)) for k in ("position", "normal", "albedo")]

    before = snapshot()
    for k in range(2):
        _view(r, k, size)
        r.render()
        r.post(pcfg(R | T))
    after = snapshot()
    for x, y in zip(before, after):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert (bits(r.downloadPostColor()) != bits(before[0])).any()          # (the chain's result is another frame)
    assert debug_buffer(r, "post_color")[1] >= w * h * 16
    # a context that steps through the separate calls never makes post buffers
    r2 = _atrium(size, cfg_foveated(12, 36, (1, 2, 4)))
    r2.render()
    separate(r2, pcfg(D | R | T | M))
    r2.synchronize()
    with pytest.raises(lib.FovptError) as e:
        debug_buffer(r2, "post_color")
    assert e.value.code == E_INVALID
    for q in (r, r2):
        q.close()


# ---- 6. ordering --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["frames_in_flight", "chains_per_frame"])
def test_post_is_ordered_with_frames_in_flight(mode):
    """Update, render and fovpt_post issued back to back over four frames, no synchronisation in between, into caller buffers: what
    the same sequence gives with a synchronise after every call."""
    import torch
    size = (384, 216)
    cfg = cfg_foveated(20, 60, (4, 8, 16))               # >= 16384 sample slots: chains_per_frame = 2 does split the frame
    if mode == "frames_in_flight":
        cfg.frames_in_flight = 2
    else:
        cfg.chains_per_frame = 2
    r = _atrium(size, cfg)
    orig = {k: m.vertex for k, m in enumerate(r.model.meshes)}
    nm = len(orig)
    views = [((120 + 40 * k, 90 + 15 * k), k) for k in range(4)]
    moves = [{m: jitter(orig[m], 100 * k + m, 25.0) for m in range(nm) if (m + k) % 3 == 0} for k in range(4)]
    dev = [{m: torch.from_numpy(v).cuda() for m, v in mv.items()} for mv in moves]
    torch.cuda.synchronize()

    def setup(g, k):
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = g
        r.launchParams.frame.subframe_index = 0
        _view(r, k, size)

    def begin():
        # the meshes where they started, the accum buffer's leftovers where no pass writes as all four views leave them, no history
        r.update_vertices(orig)
        for g, k in views:
            setup(g, k)
            r.render()
        r.temporal_reset()

    pc = pcfg(R | T | M, temporal=ALL_CAPS)
    outs = [[(torch.empty((size[1], size[0], 4), dtype=torch.float32, device="cuda"), torch.empty((size[1], size[0]), dtype=torch.int32, device="cuda"),
              torch.empty((size[1], size[0], 4), dtype=torch.float32, device="cuda")) for _ in views] for _ in range(2)]
    torch.cuda.synchronize()
    hists = []
    for sync, out in zip((True, False), outs):
        begin()
        for ((g, k), (oc, op, om)) in zip(views, out):
            r.update_vertices(dev[k] if k & 1 else moves[k])   # device pointers and host arrays in turn
            if sync:
                r.synchronize()
            setup(g, k)
            r.render_async()
            if sync:
                r.synchronize()
            r.post(pc, None, oc.data_ptr(), op.data_ptr(), om.data_ptr())
            if sync:
                r.synchronize()
        r.synchronize()
        hists.append(r.downloadTemporalHistory())
    for want, got in zip(*outs):
        for x, y in zip(want, got):
            assert np.array_equal(x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32))
    assert np.array_equal(bits(hists[0]), bits(hists[1]))
    assert (hists[0][..., 3] > 1).mean() > 0.5 and (outs[0][-1][2].cpu().numpy()[..., 3] == 1).mean() > 0.5
    r.close()


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------------
def _bad_configs():
    """(label, PostConfig) of every out-of-range config value, each stage's own, with all four stages on."""
    ALL = D | R | T | M
    out = [("stages 0", pcfg(0)), ("stages 16", pcfg(16)), ("stages 31", pcfg(31)), ("M alone", pcfg(M)), ("R | M", pcfg(R | M)), ("D | M", pcfg(D | M))]
    for i in range(3):
        c = pcfg(ALL)
        c._reserved[i] = 1
        out.append(("_reserved[%d]" % i, c))
    nan, inf = float("nan"), float("inf")
    for k in ("iterations_fovea", "iterations_middle", "iterations_periphery", "iterations_uniform"):
        out += [("denoise %s %d" % (k, v), pcfg(ALL, denoise={k: v})) for v in (-1, abi.DENOISE_MAX_ITERATIONS + 1)]
    for k in ("color_sigma", "normal_sigma", "albedo_sigma"):
        out += [("denoise %s %g" % (k, v), pcfg(ALL, denoise={k: v})) for v in (0.0, nan, inf, abi.SIGMA_MAX * 2)]
    out += [("reconstruct support %g" % v, pcfg(ALL, reconstruct=dict(support=v))) for v in (0.5, 2.5, nan)]
    for k in ("normal_sigma", "depth_sigma"):
        out += [("reconstruct %s %g" % (k, v), pcfg(ALL, reconstruct={k: v})) for v in (0.0, nan, inf)]
    out += [("reconstruct levels %d" % v, pcfg(ALL, reconstruct=dict(levels=v))) for v in (-1, 4)]
    out += [("reconstruct remodulate %d" % v, pcfg(ALL, reconstruct=dict(remodulate=v))) for v in (-1, 2)]
    for i in range(3):
        c = pcfg(ALL)
        c.reconstruct._reserved[i] = 1
        out.append(("reconstruct _reserved[%d]" % i, c))
    Mh = abi.TEMPORAL_MAX_HISTORY
    for k in ("history_fovea", "history_middle", "history_periphery", "history_uniform"):
        out += [("temporal %s %d" % (k, v), pcfg(ALL, temporal={k: v})) for v in (0, -1, Mh + 1)]
    for k, top in (("normal_tolerance", 4), ("depth_tolerance", 1)):
        out += [("temporal %s %g" % (k, v), pcfg(ALL, temporal={k: v}))
                for v in (-1e-7, nan, inf, float(np.nextafter(np.float32(top), np.float32(top + 1))))]
    for i in range(2):
        c = pcfg(ALL)
        c.temporal._reserved[i] = 1
        out.append(("temporal _reserved[%d]" % i, c))
    return out


def test_post_errors_are_all_or_nothing():
    """Every rejected call returns its code; the valid call that follows it is bit for bit the one on a twin context that never saw
    the failure: nothing was enqueued, no state (history set, tracking, epoch) moved."""
    import torch
    size = (96, 64)
    ALL = D | R | T | M
    a, b = (_cornell(size, cfg_foveated(10, 24, (1, 2, 4))) for _ in range(2))
    good = pcfg(ALL, temporal=ALL_CAPS)
    motions = cornell_motions(a.model)
    count = [0]

    def refuse(code, label, *args):
        with pytest.raises(lib.FovptError) as e:
            b.post(*args)
        assert e.value.code == code, label

    def agree(label):
        for r in (a, b):
            r.post(good, out_motion=r.motion_buffer())
        same(a, b, ALL, label, stepped=True, a_posts=True)
        count[0] += 1

    def refused(code, label, *args):
        """b refuses post(*args) with `code`; then both take a valid step and agree."""
        refuse(code, label, *args)
        agree(label)

    with pytest.raises(lib.FovptError) as e:                 # nothing rendered yet
        b.post()
    assert e.value.code == E_NO_FRAME
    for k in range(2):                                       # two ordinary steps, a mesh moved in between: tracking is on
        for r in (a, b):
            if k:
                r.update_vertices(motions[0][1])
            _cornell_view(r, k, size)
            r.render()
            r.post(good, out_motion=r.motion_buffer())
        same(a, b, ALL, "step %d" % k, a_posts=True)
    for r in (a, b):                                         # a frame with a moved mesh to step on while calls are refused
        r.update_vertices(motions[1][1])
        _cornell_view(r, 2, size)
        r.render()
    for label, c in _bad_configs():
        refused(E_INVALID, label, c, None, None, None, b.motion_buffer() if c.stages & M else None)
    mo, f = b.motion_buffer(), b.launchParams.frame
    col, rgba, hist = b.temporal_buffers()
    pcol, prgba = b.post_buffers()
    dcol = b.denoise_buffers()[0]
    other = b.reconstruct_buffers()[0]                       # (a float4 frame of the context's that the chain does not use)
    RTM = pcfg(R | T | M)
    refused(E_INVALID, "out_motion without MOTION", pcfg(R | T), None, None, None, mo)
    refused(E_INVALID, "out_motion with DENOISE alone", pcfg(D), None, None, None, mo)
    refused(E_INVALID, "in_color with DENOISE", pcfg(ALL), other)
    refused(E_INVALID, "in_color with DENOISE alone", pcfg(D), other)
    refused(E_INVALID, "out_color is the reconstruction's input", RTM, other, other)
    refused(E_INVALID, "out_color is the accum buffer it reconstructs", RTM, None, f.accum_buffer)
    refused(E_INVALID, "out_color is the reconstruction's input (R alone)", pcfg(R), other, other)
    refused(E_INVALID, "out_color is the denoiser's output, which it reconstructs", pcfg(ALL), None, dcol)
    refused(E_INVALID, "out_color is the history", RTM, None, hist)
    refused(E_INVALID, "out_motion is out_color", RTM, None, other, None, other)
    refused(E_INVALID, "out_motion is out_rgba", RTM, None, None, mo, mo)
    refused(E_INVALID, "out_motion is the input", RTM, mo, None, None, mo)
    refused(E_INVALID, "out_motion is the accum buffer", RTM, None, None, None, f.accum_buffer)
    refused(E_INVALID, "out_motion is the history", RTM, None, None, None, hist)
    refused(E_INVALID, "out_motion is the context's own output", RTM, None, None, None, pcol)
    refused(E_INVALID, "out_motion is the albedo guide the fused kernel reads", RTM, None, None, None, f.albedo_buffer)
    other_hist = b.temporal_buffers()[2]                     # (the valid steps in between have turned the sets)
    for h_ in {hist, other_hist}:
        refused(E_INVALID, "out_color is a history", RTM, None, h_)
        refused(E_INVALID, "out_motion is a history", RTM, None, None, None, h_)
    f.size.x -= 4
    for st in (ALL, R | T | M, T, R, D):
        refuse(E_NO_FRAME, "another frame size", pcfg(st))
    f.size.x += 4
    agree("another frame size")
    trav = b.launchParams.traversable
    b.launchParams.traversable = 12345
    for st in (ALL, R | T | M, T, R):
        refuse(E_NO_SCENE, "another traversable", pcfg(st))
    b.launchParams.traversable = trav
    agree("another traversable")
    for name in ("accum_buffer", "albedo_buffer", "color_buffer", "normal_buffer"):
        keep = getattr(f, name)
        setattr(f, name, None)
        refuse(E_INVALID, "null " + name, pcfg(R | T | M) if name == "accum_buffer" else good)
        setattr(f, name, keep)
        agree("null " + name)
    L = lib.load()
    assert L.fovpt_post(b._ctx, None, C.byref(good), None, None, None, None) == E_INVALID
    assert L.fovpt_post(b._ctx, C.byref(b.launchParams), None, None, None, None, None) == E_INVALID
    col_, rgba_ = C.c_void_p(), C.c_void_p()
    assert L.fovpt_post_buffers(b._ctx, None, C.byref(rgba_)) == E_INVALID and L.fovpt_post_buffers(b._ctx, C.byref(col_), None) == E_INVALID
    refused(E_INVALID, "(after the null arguments)", pcfg(0))
    # frames the chain cannot take: both contexts render them, only b asks
    for what in ("world", "guides"):
        for r in (a, b):
            c = r.config
            if what == "world":
                c.world, c.rank = 2, 0
            else:
                c.write_guides = 0
            r.config = c
            r.render()
        for st in ((ALL, R | T | M, T, R, D) if what == "world" else (ALL, D, R | T | M, R)):
            with pytest.raises(lib.FovptError) as e:         # a tile shard; no guides for DENOISE or remodulate = 1
                b.post(pcfg(st))
            assert e.value.code == E_INVALID, (what, st)
        for r in (a, b):
            c = r.config
            c.world, c.rank, c.write_guides = 1, 0, 1
            r.config = c
            r.render()
            r.post(good, out_motion=r.motion_buffer())
        same(a, b, ALL, what, stepped=True, a_posts=True)
    assert (b.downloadTemporalHistory()[..., 3] > 1).mean() > 0.5 and count[0] >= len(_bad_configs())
    torch.cuda.synchronize()
    a.close()
    b.close()


# ---- 8. the C++ drop-in -------------------------------------------------------------------------------------------------------------
def test_cpp_dropin_post(tmp_path):
    """SampleRenderer::post() + downloadPostPixels / downloadMotion of include/SimplePathtracer.h: the same pixels and motion
    vectors as Python."""
    exe, out = build_dropin(tmp_path, "post_gpu_test"), str(tmp_path / "post_out.bin")
    run_dropin(exe, out)
    n = 160 * 96
    raw = np.fromfile(out, np.uint32)
    px = raw[:2 * n].reshape(2, 96, 160)
    mv = raw[2 * n:].view(np.float32).reshape(96, 160, 4)
    r = dropin_renderer(write_guides=True)
    model = r.model
    r.render()
    r.post()
    assert np.array_equal(px[0], r.downloadPostPixels())
    r.update_vertices({1: (model.meshes[1].vertex + np.float32([0.5, 0.0, -0.25])).astype(np.float32)})
    r.render()
    r.post(out_motion=r.motion_buffer())
    assert np.array_equal(px[1], r.downloadPostPixels())
    assert np.array_equal(bits(mv), bits(r.downloadMotion()))
    box = r.downloadGBuffer()["prim"]
    box = (box != tr.MISS) & (box >= len(model.meshes[0].index))
    assert box.sum() > 100 and (np.abs(mv[box][:, :2]).max(axis=-1) > 1).mean() > 0.5   # the box's pixels did move
    r.close()
