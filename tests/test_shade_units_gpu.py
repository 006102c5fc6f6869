"""k_shade's probe lookup, Disney BSDF and texture fetch, input by input (csrc/fovpt_shade_fn.h, csrc/fovpt_scene.h through
csrc/shade_debug.hip): the device functions on the inputs of tests/shade_cases.py against the oracle in detmath mode, compared
as bits; where the oracle's value is NaN the device's must be NaN.  tests/test_shade_units_cpu.py shows without a GPU what
these inputs reach.

The probe entry points search the probe the way a launch of the context would, and say which layout that was: the guided
search over packed records for the varied probes, one row of the split arrays for the probes whose rows are alike, the
reference's plain binary search for the probe with negative texels -- and the plain search on the same arrays must give
the same answer as whichever layout ran.  One test ties the unit level to a frame's seeding and draws: the shadow rays a
32 x 32 frame queued at its first hits carry exactly the directions the entry point returns for the numbers those paths drew."""
import ctypes as C

import numpy as np
import pytest

import shade_cases as sc
from common import cfg_uniform, make_gpu
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer, scenes
from gpu_common import debug_buffer

pytestmark = pytest.mark.gpu


def _model():
    m = scenes.cornell_box()
    m.textures.extend(sc.textures())
    return m


@pytest.fixture(scope="module")
def r():
    rr = renderer.SampleRenderer(_model())
    yield rr
    rr.close()


def _same(what, got, want):
    """Bit-equal, or NaN where the oracle has NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.dtype == np.float32:
        nan = np.isnan(want)
        bad = np.where(nan, ~np.isnan(got), got.view(np.uint32) != want.view(np.uint32))
    else:
        bad = got != want
    idx = np.argwhere(bad)
    assert idx.size == 0, (what, len(idx), idx[:6].tolist(), got[bad][:6], want[bad][:6])


@pytest.mark.parametrize("case", sc.probe_cases(), ids=lambda c: c.name)
def test_probe_sample(oracle, r, case):
    hp, r12, want = sc.probe_reference(oracle, case)
    assert want["row"].min() >= 0 and want["row"].max() < case.height and want["col"].min() >= 0 and want["col"].max() < case.width
    case.install(r)
    got = r.debug_probe_sample(r12)
    plain = r.debug_probe_sample(r12, plain=True)
    print(case.name, len(r12), "pairs, layout", got["path"])
    assert got["path"] == case.path and plain["path"] == sc.PATH_PLAIN
    for k in ("row", "col", "dir", "color", "pdf"):
        _same((case.name, k), got[k], want[k])
        _same((case.name, "plain", k), plain[k], want[k])
        assert np.array_equal(got[k].view(np.uint32), plain[k].view(np.uint32)), (case.name, k)


@pytest.mark.parametrize("case", sc.probe_cases(), ids=lambda c: c.name)
def test_probe_eval(oracle, r, case):
    hp = case.host_probe(oracle)
    d = sc.probe_directions(case.width, case.height)
    want = oracle.probe_eval(hp, d)
    case.install(r)
    got = r.debug_probe_eval(d)
    plain = r.debug_probe_eval(d, plain=True)
    assert got["path"] == case.path and plain["path"] == sc.PATH_PLAIN
    for k in ("uv", "texel"):
        _same((case.name, k), got[k], want[k])
        _same((case.name, "plain", k), plain[k], want[k])


def test_a_foreign_probe_is_searched_plainly(oracle, r):
    """The guide tables belong to the probe the context uploaded: the same arrays under another size are a probe of the
    caller's own, and get the reference's search."""
    case = [c for c in sc.probe_cases() if c.name == "sky96x40"][0]
    mine = case.install(r)
    other = abi.Probe.from_buffer_copy(mine)
    other.width, other.height = 48, 20                      # (inside the uploaded arrays: 48 x 20 of 96 x 40)
    hp = case.host_probe(oracle)
    cut = case.host_probe(oracle)                           # (the same arrays under the other size, as on the device)
    cut.struct.width, cut.struct.height = 48, 20
    r12 = sc.probe_pairs(hp)[::9]
    want = oracle.probe_sample_at(cut, r12)
    ok = (want["row"] < 20) & (want["col"] < 48)             # the cut tables are no CDFs: keep the pairs whose searches stay inside
    assert ok.sum() > 100
    got = r.debug_probe_sample(r12[ok], probe=other)
    assert got["path"] == sc.PATH_PLAIN
    for k in ("row", "col", "dir", "color", "pdf"):
        _same(("foreign", k), got[k], want[k][ok])


@pytest.mark.parametrize("name", [m[0] for m in sc.bsdf_materials()])
def test_bsdf(oracle, r, name):
    tables = [t for t in sc.bsdf_tables(oracle) if t[0] == name]
    assert len(tables) == len(sc.ETAS)
    for _, mat, eta_i, eta_o, g, want in tables:
        n = sc.BSDF_ROWS
        got = r.debug_bsdf(mat, g["N"], g["view"], g["albedo"], np.full(n, eta_i, np.float32), np.full(n, eta_o, np.float32), g["seeds"], g["L_given"])
        for k in ("rng_after", "light", "pdf", "eval", "pdf_again", "eval_given", "pdf_given"):
            _same((name, eta_i, eta_o, k), got[k], want[k])


@pytest.mark.parametrize("k", range(len(sc.TEXTURE_SIZES)), ids=["%dx%d" % s for s in sc.TEXTURE_SIZES])
def test_tex2d(oracle, r, k):
    tex = sc.textures()[k]
    uv = sc.texture_coordinates(tex.shape[1], tex.shape[0])
    want = oracle.tex2d(tex, uv)
    assert np.isnan(want).any() and np.isfinite(want).any()
    _same(("tex2d", k), r.debug_tex2d(k, uv), want)


def test_entry_points_refuse_bad_arguments(r):
    L, ctx = r._L, r._ctx
    case = sc.probe_cases()[2]
    p = case.install(r)
    one = np.float32([[0.5, 0.5]])
    out = np.empty(16, np.float32)
    rc = np.empty(2, np.int32)

    E_INVALID, E_NO_SCENE, E_NO_PROBE = -1, -3, -4
    assert L.fovpt_debug_probe_sample(None, C.byref(p), 0, 1, one.ctypes.data, rc.ctypes.data, out.ctypes.data, None) == E_INVALID
    assert L.fovpt_debug_probe_sample(ctx, None, 0, 1, one.ctypes.data, rc.ctypes.data, out.ctypes.data, None) == E_INVALID
    assert L.fovpt_debug_probe_sample(ctx, C.byref(p), 0, -1, one.ctypes.data, rc.ctypes.data, out.ctypes.data, None) == E_INVALID
    assert L.fovpt_debug_probe_sample(ctx, C.byref(p), 0, 1, None, rc.ctypes.data, out.ctypes.data, None) == E_INVALID
    assert L.fovpt_debug_probe_sample(ctx, C.byref(p), 2, 1, one.ctypes.data, rc.ctypes.data, out.ctypes.data, None) == E_INVALID
    for bad in (1.0, -1e-9, np.nan, np.inf):
        with pytest.raises(lib.FovptError) as e:
            r.debug_probe_sample(np.float32([[0.25, bad]]))
        assert e.value.code == E_INVALID
    empty = abi.Probe()
    with pytest.raises(lib.FovptError) as e:
        r.debug_probe_sample(one, probe=empty)
    assert e.value.code == E_NO_PROBE
    with pytest.raises(lib.FovptError) as e:
        r.debug_probe_eval(np.float32([[0, 1, 0]]), probe=empty)
    assert e.value.code == E_NO_PROBE
    assert L.fovpt_debug_probe_eval(ctx, C.byref(p), 0, 1, None, out.ctypes.data, None) == E_INVALID
    assert L.fovpt_debug_bsdf(ctx, None, 0, None, None, None, None, None, None, None, None) == E_INVALID
    mat = abi.Material.reference_default()
    assert L.fovpt_debug_bsdf(ctx, C.byref(mat), 1, None, None, None, None, None, None, None, out.ctypes.data) == E_INVALID
    assert L.fovpt_debug_bsdf(ctx, C.byref(mat), 0, None, None, None, None, None, None, None, None) == 0
    for bad in (-1, len(sc.TEXTURE_SIZES), 1 << 20):
        with pytest.raises(lib.FovptError) as e:
            r.debug_tex2d(bad, one)
        assert e.value.code == E_INVALID
    assert L.fovpt_debug_tex2d(ctx, 0, 1, None, out.ctypes.data) == E_INVALID
    bare = C.c_void_p()
    lib.check(None, L.fovpt_create(C.byref(bare), 0))
    try:
        assert L.fovpt_debug_tex2d(bare, 0, 1, one.ctypes.data, out.ctypes.data) == E_NO_SCENE
    finally:
        L.fovpt_destroy(bare)
    # and a good call still works afterwards
    assert r.debug_probe_sample(one)["path"] == case.path


def test_a_frames_probe_samples_are_the_entry_points(oracle):
    """A 32 x 32 uniform frame, one sample per pixel, depth 1.  Sample slot = pixel; its generator is Random(tea4(pixel, 0)) -- a
    uniform frame renders subframe 0 (SimplePathtracer.cpp:87) --
    and the first two numbers it draws are the probe sample of the first hit (deviceProgram.cu:411, :303).  Every shadow ray
    the frame queued at bounce 0 -- origin.w = slot, direction = the probe sample's -- must carry the direction
    debug_probe_sample returns for those two numbers, which is also the oracle's ProbeSample for that seed.  This ties the
    seeding, the order of the draws and the probe the launch read to the unit level.  It cannot tell which layout the launch
    searched -- every layout returns the same sample, which is what the tests above hold -- that the launch and the entry
    point choose the same one is the shared probe_path() of fovpt_api.hip, which the entry points of api_debug.hip call."""
    w = h = 32
    data = scenes.sky_probe(96, 40)
    r = make_gpu(scenes.cornell_box(), data, scenes.CORNELL_CAMERA, (w, h), cfg_uniform(1, 1))
    with open("/proc/self/maps") as f:               # the HIP runtime libfovpt.so is bound to, whatever its version
        loaded = sorted({line.split()[-1] for line in f if "libamdhip64.so" in line})
    assert len(loaded) == 1, loaded
    hip = C.CDLL(loaded[0])
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    try:
        # the state sets rotate from job to job: fill each set's shadow queue with 0xff before the job that we read, so that
        # every entry with a slot below w * h is one this frame wrote
        seen = set()
        for _ in range(10):
            r.launchParams.frame.subframe_index = 0
            r.render()
            po, no = debug_buffer(r, "sq_o")
            if po in seen:
                break
            seen.add(po)
            assert hip.hipMemset(po, 0xff, no) == 0
        else:
            pytest.fail("the state sets never came round")
        pd, nd = debug_buffer(r, "sq_d")
        so = r.download(po, np.empty((no // 16, 4), np.float32))
        sd = r.download(pd, np.empty((nd // 16, 4), np.float32))
        slot = so[:, 3].copy().view(np.uint32)
        live = np.flatnonzero(slot < w * h)
        print("shadow rays of the frame:", len(live))
        assert len(live) > 200 and len(np.unique(slot[live])) == len(live)
        seeds = [oracle.tea4(int(s), 0) for s in slot[live]]
        r12 = np.float32([oracle.random_stream(s, 2)[1] for s in seeds])
        got = r.debug_probe_sample(r12)
        assert got["path"] == sc.PATH_GUIDED | sc.PATH_RECORDS
        _same("frame: shadow direction", sd[live, :3], got["dir"])
        assert (sd[live, 3].copy().view(np.uint32) == 0).all()             # the radiance cell of depth 0
        hp = oracle.HostProbe(data)
        for k in range(0, len(live), 7):
            s = seeds[k]
            d, c, p = oracle.probe_sample(hp, s if s < 0x80000000 else s - (1 << 32), 1)
            _same("frame: oracle", got["dir"][k], d[0])
            _same("frame: oracle pdf", got["pdf"][k:k + 1], p)
    finally:
        r.close()
