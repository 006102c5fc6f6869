"""fovpt_quality on the GPU against tests/quality_ref.py, bit for bit in every field: rendered Cornell frames foveated and FOV_OFF,
tiny frames, frames whose tiles, aprons and windows cross tile edges, gazes in a corner and off the frame, a frame of many blocks,
the device against the host implementation, ordering with frames and measurements in flight, the buffers it must leave alone,
every rejection, a seeded sweep, and the C++ drop-in.  The test and reference images are random codes uploaded by the tests; the
frame description (passes, gaze, FOV_OFF) is the rendered one."""
import ctypes as C
import os

import numpy as np
import pytest

import quality_cases as qc
import quality_ref as qr
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer, scenes

from common import cfg_foveated, cfg_uniform, make_gpu
from gpu_common import bits, build_dropin, device_filled, dropin_renderer, run_dropin, upload, with_entries

pytestmark = pytest.mark.gpu
E_INVALID, E_NO_FRAME = -1, -5
CORNELL = scenes.CORNELL_CAMERA
PROBE = scenes.ambient_probe(64, 32, 2.0)
SIZE = (64, 48)
ALL_FLAGS = [0, qr.SSIM, qr.PROFILE, qr.SSIM | qr.PROFILE]
SUMS_BYTES = C.sizeof(abi.QualitySums)


def _cornell(size=SIZE, cfg=None, gaze=None):
    cfg = cfg if cfg is not None else cfg_foveated(6, 14, (1, 1, 2))
    cfg.write_guides = 1
    return make_gpu(scenes.cornell_box(), PROBE, CORNELL, size, cfg, gaze=gaze)


def sums_of(t):
    """The abi.QualitySums a device record (a uint8 tensor) holds."""
    return abi.QualitySums.from_buffer_copy(t.cpu().numpy().tobytes())


def qcfg(d=None):
    """fovpt_quality_defaults with the entries of d replaced -> (abi.QualityConfig, the dict for the restatement)."""
    c = with_entries(renderer.SampleRenderer.quality_defaults(), d)
    return c, dict(flags=c.flags, ring_width=c.ring_width)


def frame_classes(r):
    """The classes of the frame r rendered last (r.launchParams and r.config as at render time), from reconstruct_ref.writers."""
    f, cfg = r.launchParams.frame, r.config
    return qr.classes_of_frame(f.size.x, f.size.y, (f.c.x, f.c.y), cfg.r_inner, cfg.r_outer, cfg.uniform)


def random_pair(rng, w, h, near=True):
    """Two images of random codes; near: the second is the first with small errors in places, so that SSIM is not all noise."""
    a = rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
    if not near:
        return a, rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
    ch = a.view(np.uint8).reshape(h, w, 4).astype(np.int64)
    ch = np.clip(ch + rng.integers(-9, 10, ch.shape) * (rng.random((h, w, 1)) < 0.6), 0, 255).astype(np.uint8)
    return a, np.ascontiguousarray(ch).view(np.uint32).reshape(h, w)


def check(r, test, ref, d=None, classes=None, label=None):
    """One measurement into a record and a class map of the caller's: the record is the restatement's bit for bit, the class map is
    the one derived from the writers, and the host implementation fed that class map gives the record too."""
    f = r.launchParams.frame
    w, h = f.size.x, f.size.y
    c, full = qcfg(d)
    dt, dr = upload(test), upload(ref)
    out, cls = device_filled(SUMS_BYTES, 0xa5), device_filled(w * h, 0xee)
    r.qualityAsync(dr.data_ptr(), dt.data_ptr(), c, out.data_ptr(), cls.data_ptr())
    r.synchronize()
    got, got_cls = sums_of(out), cls.cpu().numpy().reshape(h, w)
    classes = classes if classes is not None else frame_classes(r)
    assert np.array_equal(got_cls, classes), label
    gaze = (f.c.x, f.c.y)
    want = qr.quality(test, ref, classes, gaze, full)
    assert got.as_dict() == want, label
    assert bytes(got) == bytes(qc.sums_of_dict(want)), label              # (every byte: the padding too)
    rc, host = qc.host_quality(lib.load(), test, ref, got_cls, gaze, full)
    assert rc == 0 and bytes(host) == bytes(got), label
    return want, classes


# ---- 1. rendered frames -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("uniform", [False, True], ids=["foveated", "fov_off"])
def test_rendered_cornell_frames(uniform):
    r = _cornell(cfg=cfg_uniform(2) if uniform else None)
    r.render()
    rng = np.random.default_rng(21 + uniform)
    classes = frame_classes(r)
    seen = set(np.unique(classes).tolist())
    assert seen == ({qr.UNIFORM} if uniform else {qr.FOVEA, qr.MIDDLE, qr.PERIPHERY, qr.UNWRITTEN})
    for flags in ALL_FLAGS:
        for rw in (1, 7, 65536):
            test, ref = random_pair(rng, *SIZE)
            want, _ = check(r, test, ref, dict(flags=flags, ring_width=rw), classes, (flags, rw))
            assert (sum(want["windows"]) > 0) == bool(flags & qr.SSIM) and (sum(want["ring_pixels"]) > 0) == bool(flags & qr.PROFILE)
    # the same image twice, and the same buffer twice: no error, every window's q is 2^20
    test, _ = random_pair(rng, *SIZE)
    want, _ = check(r, test, test, None, classes, "equal images")
    assert want["ssim_q20"] == [n << 20 for n in want["windows"]] and want["differing"] == [0] * 5
    dt = upload(test)
    out = device_filled(SUMS_BYTES, 0xa5)
    r.qualityAsync(dt.data_ptr(), dt.data_ptr(), None, out.data_ptr())
    r.synchronize()
    assert sums_of(out).as_dict() == want
    # test_rgba None is the frame buffer; numpy images are uploaded by the binding
    _, ref = random_pair(rng, *SIZE, near=False)
    got = r.measureQuality(ref, classes=True)
    want = qr.quality(r.downloadPixels(), ref, classes, (r.launchParams.frame.c.x, r.launchParams.frame.c.y))
    assert np.array_equal(got["classes"], classes) and {k: got[k] for k in want} == want
    assert got["mse"]["all"] == qr.mse(want) and got["psnr"]["all"] == qr.psnr(want) and got["ssim"]["all"] == qr.ssim(want)
    r.close()


# ---- 2. tiny frames -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1, 1), (3, 1), (1, 5), (4, 4), (8, 8), (11, 12)], ids=lambda s: "%dx%d" % s)
def test_tiny_frames(size):
    r = _cornell(size, cfg_foveated(1, 2, (1, 1, 1)), gaze=(0, 0))
    r.render()
    rng = np.random.default_rng(31)
    for flags in ALL_FLAGS:
        test, ref = random_pair(rng, *size)
        want, _ = check(r, test, ref, dict(flags=flags, ring_width=2), label=(size, flags))
        n_windows = 0 if min(size) < 8 else ((size[0] - 8) // 4 + 1) * ((size[1] - 8) // 4 + 1)
        assert sum(want["windows"]) == (n_windows if flags & qr.SSIM else 0)
    r.config = cfg_uniform(1)
    r.render()
    test, ref = random_pair(rng, *size)
    want, classes = check(r, test, ref, label=(size, "fov_off"))
    assert (classes == qr.UNIFORM).all() and want["pixels"][qr.UNIFORM] == size[0] * size[1]
    r.close()


# ---- 3. tiles, aprons and windows that cross tile edges; gazes in a corner and off the frame ------------------------------------------
@pytest.mark.parametrize("size", [(70, 45), (61, 37)], ids=lambda s: "%dx%d" % s)
def test_frames_of_several_tiles_and_odd_sizes(size):
    w, h = size
    r = _cornell(size)
    rng = np.random.default_rng(41)
    u32 = lambda v: v & 0xffffffff
    cases = [("in the frame", (w // 2, h // 2), False), ("at a corner", (0, 0), False), ("at the last pixel", (w - 1, h - 1), False),
             ("off the frame", (w + 40, h + 40), False), ("far off the frame", (4000, 3000), False), ("wrapped", (u32(-5), u32(-3)), False),
             ("FOV_OFF", (w // 2, h // 2), True)]
    seen = set()
    for k, (label, gaze, uniform) in enumerate(cases):
        cfg = cfg_uniform(1) if uniform else cfg_foveated(6, 14, (1, 1, 2))
        r.config = cfg
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = gaze
        r.render()
        test, ref = random_pair(rng, w, h, near=k % 2 == 0)
        want, classes = check(r, test, ref, dict(ring_width=(1, 3, 16)[k % 3]), label=label)
        seen |= set(np.unique(classes).tolist())
        assert sum(want["windows"]) == ((w - 8) // 4 + 1) * ((h - 8) // 4 + 1) and sum(want["ring_pixels"]) == w * h
    assert seen == {0, 1, 2, 3, 4}
    r.close()


# ---- 4. many blocks -------------------------------------------------------------------------------------------------------------------
def test_a_frame_of_many_blocks():
    """1920 x 1080: 2040 tiles over the capped grid, so a block strides over tiles and its columns go beyond 32 bits' worth of a
    tile."""
    size = (1920, 1080)
    r = _cornell(size, cfg_foveated(74, 241, (1, 1, 1)), gaze=(1000, 500))
    r.render()
    rng = np.random.default_rng(7)
    test, ref = random_pair(rng, *size, near=False)
    want, classes = check(r, test, ref)
    assert {qr.FOVEA, qr.MIDDLE, qr.PERIPHERY} <= set(np.unique(classes).tolist())
    assert max(max(c) for c in want["sq_err"]) > 1 << 32 and sum(want["windows"]) == 479 * 269
    r.close()


# ---- 5. ordering ------------------------------------------------------------------------------------------------------------------------
def test_quality_measures_the_frame_that_was_rendered_with_frames_in_flight():
    """render_async, quality of the frame buffer, render_async, quality ... with no synchronisation in between: what the same
    sequence gives with a synchronise after every call, which is the restatement of each frame's own frame buffer and gaze."""
    size = (384, 216)
    cfg = cfg_foveated(20, 60, (4, 8, 16))
    cfg.frames_in_flight = 2
    r = _cornell(size, cfg)
    views = [((120, 90), 0), ((300, 40), 1), ((30, 200), 2)]
    rng = np.random.default_rng(51)
    ref = rng.integers(0, 1 << 32, (size[1], size[0]), dtype=np.uint64).astype(np.uint32)
    dref = upload(ref)
    c, full = qcfg(dict(ring_width=9))

    def setup(g, k):
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = g
        r.launchParams.frame.subframe_index = k

    results = []
    for sync in (True, False):
        for g, k in views:                                   # the frame buffer's leftovers where no pass writes, as all views leave them
            setup(g, k)
            r.render()
        outs = [(device_filled(SUMS_BYTES, 0xa5), device_filled(size[0] * size[1], 0xee)) for _ in views]
        for (g, k), (out, cls) in zip(views, outs):
            setup(g, k)
            r.render_async()
            if sync:
                r.synchronize()
                frame = r.downloadPixels()
            r.qualityAsync(dref.data_ptr(), None, c, out.data_ptr(), cls.data_ptr())
            if sync:
                r.synchronize()
                classes = frame_classes(r)
                assert np.array_equal(cls.cpu().numpy().reshape(size[1], size[0]), classes)
                assert sums_of(out).as_dict() == qr.quality(frame, ref, classes, g, full)
        r.synchronize()
        results.append([(bytes(sums_of(out)), cls.cpu().numpy().tobytes()) for out, cls in outs])
    assert results[0] == results[1]
    assert len({s for s, _ in results[0]}) == 3 and len({k for _, k in results[0]}) == 3          # (the frames differ)
    r.close()


def test_measurements_in_flight_and_the_contexts_own_record():
    r = _cornell()
    r.render()
    rng = np.random.default_rng(61)
    classes = frame_classes(r)
    gaze = (r.launchParams.frame.c.x, r.launchParams.frame.c.y)
    jobs = []
    for k, d in enumerate((dict(flags=qr.SSIM), dict(flags=qr.PROFILE, ring_width=2), dict(ring_width=30))):
        test, ref = random_pair(rng, *SIZE, near=k != 1)
        jobs.append((test, ref, qcfg(d), upload(test), upload(ref), device_filled(SUMS_BYTES, 0xa5)))
    for test, ref, (c, _), dt, dr, out in jobs:              # three calls back to back, nothing in between
        r.qualityAsync(dr.data_ptr(), dt.data_ptr(), c, out.data_ptr())
    r.synchronize()
    wants = [qr.quality(test, ref, classes, gaze, full) for test, ref, (_, full), _, _, _ in jobs]
    for (_, _, _, _, _, out), want in zip(jobs, wants):
        assert sums_of(out).as_dict() == want
    assert len({bytes(sums_of(j[5])) for j in jobs}) == 3
    # out_sums NULL: the context's own record, which fovpt_quality_read returns; the caller's records stay
    assert bytes(r.readQuality(sums=True)) == bytes(SUMS_BYTES)                                   # (none yet: zeros)
    test, ref, (c, full), dt, dr, _ = jobs[1]
    r.qualityAsync(dr.data_ptr(), dt.data_ptr(), c)
    r.qualityAsync(jobs[2][4].data_ptr(), jobs[2][3].data_ptr(), jobs[2][2][0], jobs[0][5].data_ptr())   # a later call into a caller's record
    got = r.readQuality()
    assert {k: got[k] for k in wants[1]} == wants[1] and got["mse"]["all"] == qr.mse(wants[1])
    assert sums_of(jobs[0][5]).as_dict() == wants[2] and sums_of(jobs[1][5]).as_dict() == wants[1]
    # the record survives fovpt_resize; the rows follow the frame
    r.resize((200, 120))
    r.setCamera(r.lastSetCamera)
    assert bytes(r.readQuality(sums=True)) == bytes(qc.sums_of_dict(wants[1]))
    with pytest.raises(lib.FovptError) as e:                 # (nothing rendered at this size yet)
        r.qualityAsync(dr.data_ptr())
    assert e.value.code == E_NO_FRAME
    r.launchParams.frame.c.x, r.launchParams.frame.c.y = 150, 20
    r.render()
    test, ref = random_pair(rng, 200, 120)
    check(r, test, ref, label="after resize")
    r.close()


# ---- 6. isolation -----------------------------------------------------------------------------------------------------------------------
def test_quality_leaves_the_other_stages_buffers_alone():
    size = (96, 64)
    a, b = (_cornell(size, cfg_foveated(10, 24, (1, 2, 4))) for _ in range(2))
    to = renderer.Camera((CORNELL["eye"][0] + 0.05, CORNELL["eye"][1], CORNELL["eye"][2]), CORNELL["lookat"], CORNELL["up"], CORNELL["fovy"], size[0] / size[1])

    def stages(r):
        r.denoise()
        r.reconstruct()
        r.temporal()
        r.post()
        r.expose(None, r.post_buffers()[0])
        r.focus(None, None, r.post_buffers()[0])
        r.warp(to, None, None, *r.expose_buffers())
        r.lens(None, None, r.expose_buffers()[0])

    for r in (a, b):
        r.render()
        stages(r)

    def snapshot(r):
        out = [r.downloadPostColor(), r.downloadPostPixels(), r.downloadDenoisedColor(), r.downloadDenoisedPixels(), r.downloadReconstructedColor(),
               r.downloadReconstructedPixels(), r.downloadTemporalColor(), r.downloadTemporalPixels(), r.downloadTemporalHistory(), r.downloadAccum(),
               r.downloadPixels(), r.downloadExposedColor(), r.downloadExposedPixels(), r.downloadWarpedColor(), r.downloadWarpedPixels()]
        out += list(r.downloadFocus()) + list(r.downloadLens())
        out += [np.frombuffer(bytes(s), np.uint32) for s in (r.expose_state(), r.focus_state(), r.warp_counts())]
        g = r.gbuffer()                                       # (traced again by both contexts: the same rays)
        return out + [r.download(getattr(g, k), np.empty((size[1], size[0], 4), np.float32)) for k in ("position", "normal", "albedo")]

    before = snapshot(b)
    rng = np.random.default_rng(71)
    _, ref = random_pair(rng, *size, near=False)
    first = b.measureQuality(ref, classes=True)              # the frame buffer against it, into the context's record
    b.measureQuality(b.expose_buffers()[1], b.post_buffers()[1], qcfg(dict(flags=qr.SSIM))[0])
    after = snapshot(b)
    for x, y in zip(before, after):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert sum(first["differing"]) > size[0] * size[1] // 2
    for k in range(2):                                       # the next steps equal those of the context that never measured
        for r in (a, b):
            r.launchParams.frame.c.x += 9
            r.render()
            stages(r)
        b.measureQuality(b.expose_buffers()[1])
        for x, y in zip(snapshot(a), snapshot(b)):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert bytes(a.readQuality(sums=True)) == bytes(SUMS_BYTES)                                   # and that context has no record
    for r in (a, b):
        r.close()


# ---- 7. rejections ----------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_everything_unchanged():
    r = _cornell()
    rng = np.random.default_rng(81)
    test, ref = random_pair(rng, *SIZE)
    dt, dr = upload(test), upload(ref)
    good, _ = qcfg()
    with pytest.raises(lib.FovptError) as e:                 # nothing rendered yet
        r.qualityAsync(dr.data_ptr(), dt.data_ptr())
    assert e.value.code == E_NO_FRAME
    r.render()
    r.qualityAsync(dr.data_ptr(), dt.data_ptr())             # the context's record holds a measurement
    out, cls = device_filled(SUMS_BYTES, 0x3c), device_filled(SIZE[0] * SIZE[1], 0x77)
    L = lib.load()

    def everything():
        r.synchronize()
        return bytes(r.readQuality(sums=True)), out.cpu().numpy().tobytes(), cls.cpu().numpy().tobytes()

    before = everything()
    assert before[0] != bytes(SUMS_BYTES)

    def refuse(code, label, call):
        with pytest.raises(lib.FovptError) as e:
            call()
        assert e.value.code == code, label
        assert everything() == before, label

    bad = [("flags", 4), ("flags", 8 | 1), ("flags", -1), ("flags", 1 << 31 - 1), ("ring_width", 0), ("ring_width", -1), ("ring_width", 65537),
           ("ring_width", 1 << 30)]
    for field, v in bad:
        c = good.copy()
        setattr(c, field, v)
        for sums in (out.data_ptr(), None):
            refuse(E_INVALID, (field, v), lambda: r.qualityAsync(dr.data_ptr(), dt.data_ptr(), c, sums, cls.data_ptr()))
    for i in range(6):
        c = good.copy()
        c._reserved[i] = 1
        refuse(E_INVALID, "_reserved[%d]" % i, lambda: r.qualityAsync(dr.data_ptr(), dt.data_ptr(), c, out.data_ptr(), cls.data_ptr()))
    lp = C.byref(r.launchParams)
    assert L.fovpt_quality(None, lp, C.byref(good), dt.data_ptr(), dr.data_ptr(), out.data_ptr(), cls.data_ptr()) == E_INVALID
    assert L.fovpt_quality(r._ctx, None, C.byref(good), dt.data_ptr(), dr.data_ptr(), out.data_ptr(), cls.data_ptr()) == E_INVALID
    assert L.fovpt_quality(r._ctx, lp, None, dt.data_ptr(), dr.data_ptr(), out.data_ptr(), cls.data_ptr()) == E_INVALID
    assert L.fovpt_quality(r._ctx, lp, C.byref(good), dt.data_ptr(), None, out.data_ptr(), cls.data_ptr()) == E_INVALID
    assert L.fovpt_quality_read(r._ctx, None) == E_INVALID and L.fovpt_quality_read(None, C.byref(abi.QualitySums())) == E_INVALID
    assert L.fovpt_quality_defaults(None) == E_INVALID
    assert everything() == before
    f = r.launchParams.frame
    keep = f.frame_buffer
    f.frame_buffer = None                                    # test_rgba NULL together with a null frame_buffer
    refuse(E_INVALID, "null frame_buffer", lambda: r.qualityAsync(dr.data_ptr(), None, good, out.data_ptr(), cls.data_ptr()))
    r.qualityAsync(dr.data_ptr(), dt.data_ptr(), good)       # (with a test image of the caller's the frame buffer is not looked at)
    f.frame_buffer = keep
    assert everything() == before                            # (the same measurement again)
    f.size.x -= 4
    refuse(E_NO_FRAME, "another size", lambda: r.qualityAsync(dr.data_ptr(), dt.data_ptr(), good, out.data_ptr(), cls.data_ptr()))
    f.size.x += 4
    c = r.config                                             # a tile shard does not see the frame
    c.world, c.rank = 2, 0
    r.config = c
    r.render()
    refuse(E_INVALID, "world 2", lambda: r.qualityAsync(dr.data_ptr(), dt.data_ptr(), good, out.data_ptr(), cls.data_ptr()))
    c.world, c.rank = 1, 0
    r.config = c
    r.render()
    check(r, test, ref, label="the valid call after them")
    r.close()


# ---- 8. a seeded sweep ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(int(os.environ.get("FOVPT_FUZZQ_TO", "8"))))
def test_seeded_sweep(seed):
    rng = np.random.default_rng(3000 + seed)
    w, h = int(rng.integers(1, 97)), int(rng.integers(1, 97))
    uniform = rng.random() < 0.25
    ri = int(rng.integers(0, 12))
    cfg = cfg_uniform(1) if uniform else cfg_foveated(ri, ri + int(rng.integers(0, 24)), (1, 1, 1))
    gaze = (int(rng.integers(-8, w + 8)) & 0xffffffff, int(rng.integers(-8, h + 8)) & 0xffffffff)
    r = _cornell((w, h), cfg, gaze=gaze)
    r.render()
    classes = frame_classes(r)
    for k in range(3):
        test, ref = random_pair(rng, w, h, near=rng.random() < 0.7)
        d = dict(flags=int(rng.integers(0, 4)), ring_width=int(rng.choice([1, 2, 16, 65536, int(rng.integers(1, 40))])))
        check(r, test, ref, d, classes, (seed, k, w, h, gaze, d))
    r.close()


# ---- 9. the C++ drop-in -----------------------------------------------------------------------------------------------------------------
def test_cpp_dropin_quality(tmp_path):
    """SampleRenderer::measureQuality() / qualityAsync() / readQuality() of include/SimplePathtracer.h: the same records as Python,
    which are the restatement's."""
    exe, out = build_dropin(tmp_path, "quality_gpu_test"), str(tmp_path / "quality_out.bin")
    run_dropin(exe, out)
    raw = open(out, "rb").read()
    assert len(raw) == 3 * SUMS_BYTES
    recs = [abi.QualitySums.from_buffer_copy(raw[k * SUMS_BYTES:(k + 1) * SUMS_BYTES]) for k in range(3)]
    r = dropin_renderer(gaze=(110, 38))
    r.render()
    r.lens()
    frame, lens = r.downloadPixels(), r.downloadLens()[1]
    classes = frame_classes(r)
    wants = [qr.quality(frame, lens, classes, (110, 38)), qr.quality(lens, frame, classes, (110, 38), dict(flags=qr.PROFILE, ring_width=5)),
             qr.quality(frame, frame, classes, (110, 38))]
    for k, (rec, want) in enumerate(zip(recs, wants)):
        assert rec.as_dict() == want, k
    got = r.measureQuality(r.lens_buffers()[1])
    assert {k: got[k] for k in wants[0]} == wants[0] and sum(wants[0]["differing"]) > 1000
    r.close()
