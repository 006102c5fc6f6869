"""fovpt_gather_plan / _pack / _unpack on the GPU against tests/gather_ref.py, index by index: the five kernels k_plan_owner,
k_plan_scan, k_plan_fill, k_gather_pack and k_gather_unpack (csrc/wavefront.hip) and their driver (csrc/api_gather.hip).

The plan is read through the public call alone: packing a frame that holds arange(npix) returns plan_idx itself.  No test renders
except the one that ties the plan to the renderer's own ownership.  All comparisons are exact integers.  The cases and what each
is for: tests/gather_cases.py; that they reach it: tests/test_gather_plan_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import gather_ref as gr
from fovpathtracing_optixcodelatest_amd import lib, renderer, scenes

from common import cfg_foveated, cfg_uniform, make_gpu
from gpu_common import upload
from gather_cases import CASES, IDS, random_words, restated, restated_for

pytestmark = pytest.mark.gpu
E_INVALID = -1
PACKED, PADDING, TARGET = 0xfeedc0de, 0xdeadbeef, 0x8badf00d          # three sentinels, top bit set: no index and no test word equals one
TAIL = 64


@pytest.fixture(scope="module")
def r():
    ctx = renderer.SampleRenderer(scenes.cornell_box())
    yield ctx
    ctx.close()


def configure(r, size, gaze, radii, uniform, world, tile, rank=0):
    """Resizes and reconfigures the context; the plan reads size and gaze from launchParams and the rest from the config."""
    f = r.launchParams.frame
    if (f.size.x, f.size.y) != tuple(size):
        r.resize(size)
    cfg = cfg_uniform(1) if uniform else cfg_foveated(radii[0], radii[1], (1, 1, 1))
    cfg.rank, cfg.world = rank, world
    cfg.tile_w, cfg.tile_h = tile if tile is not None else (8, 4)
    r.config = cfg
    f.c.x, f.c.y = gaze
    return cfg


def configure_case(r, case):
    return configure(r, case.size, case.gaze, case.radii, case.uniform, case.world, case.tile)


def set_rank(r, rank):
    cfg = r.config
    cfg.rank = rank
    r.config = cfg


def words(t):
    return t.cpu().numpy().view(np.uint32)


def iota_packs(r, width, height, counts):
    """Packs arange(npix) for every rank of the current plan, each into its own stretch of one sentinel-filled buffer, TAIL words
    longer than the rank's count -> per rank the (count + TAIL,) words."""
    frame = upload(np.arange(width * height, dtype=np.uint32))
    at = np.concatenate([[0], np.cumsum([c + TAIL for c in counts])]).astype(np.int64)
    buf = upload(np.full(int(at[-1]), PACKED, np.uint32))
    for rank in range(len(counts)):
        set_rank(r, rank)
        r.gather_pack(frame.data_ptr(), buf.data_ptr() + 4 * int(at[rank]))
    r.synchronize()
    set_rank(r, 0)
    got = words(buf)
    return [got[at[k]:at[k + 1]] for k in range(len(counts))]


def assert_packs_are_the_plan(packs, lists, width):
    for rank, (got, want) in enumerate(zip(packs, lists)):
        n = len(want)
        assert len(got) == n + TAIL
        if not np.array_equal(got[:n], want):
            k = int(np.flatnonzero(got[:n] != want)[0])
            g, e = int(got[k]), int(want[k])
            pytest.fail("rank %d, position %d of %d: expected pixel (%d, %d), got (%d, %d) [word 0x%08x]"
                        % (rank, k, n, e % width, e // width, g % width, g // width, g))
        assert (got[n:] == PACKED).all(), "rank %d: pack wrote past its %d words" % (rank, n)


def check_plan(r, size, gaze, radii, uniform, world, tile):
    """gather_plan for the context's current configuration, then the iota pack of every rank against the restatement."""
    owner, lists, counts = restated_for(size, gaze, radii, uniform, world, tile)
    assert r.gather_plan() == counts
    assert_packs_are_the_plan(iota_packs(r, size[0], size[1], counts), lists, size[0])
    return lists, counts


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_plan_counts(r, case):
    owner, lists, counts = restated(case)
    configure_case(r, case)
    got = r.gather_plan()
    assert got == counts
    assert r.gather_plan() == got                                          # the cached plan
    for rank in (case.world - 1, 0):                                       # every rank computes the same plan
        set_rank(r, rank)
        assert r.gather_plan() == counts


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pack_is_the_plan(r, case):
    """packed[:count] of an arange frame is the rank's restated list, element for element; the words behind it keep the sentinel,
    and a rank that owns nothing leaves the whole buffer alone."""
    owner, lists, counts = restated(case)
    configure_case(r, case)
    assert r.gather_plan() == counts
    assert_packs_are_the_plan(iota_packs(r, case.size[0], case.size[1], counts), lists, case.size[0])


# ---- unpack --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_unpack(r, case):
    owner, lists, counts = restated(case)
    npix, world = owner.size, case.world
    configure_case(r, case)
    assert r.gather_plan() == counts
    written = owner.reshape(-1) != gr.NOBODY
    top = max(counts)
    for stride in (top, (top + 63) // 64 * 64):
        gathered = np.full((world, stride), PADDING, np.uint32)
        for k in range(world):
            gathered[k, :counts[k]] = random_words(counts[k], 100 + k) >> 1          # (top bit clear: no sentinel among them)
        want = gr.unpack(gathered, stride, lists, np.full(npix, TARGET, np.uint32))
        dev, target = upload(gathered), upload(np.full(npix, TARGET, np.uint32))
        r.gather_unpack(dev.data_ptr(), stride, target.data_ptr())
        r.synchronize()
        got = words(target)
        assert (got[~written] == TARGET).all(), "unpack wrote %d pixels nobody owns" % int((got[~written] != TARGET).sum())
        assert not (got == PADDING).any() and not (got[written] == TARGET).any()
        if not np.array_equal(got, want):
            k = int(np.flatnonzero(got != want)[0])
            pytest.fail("stride %d: pixel (%d, %d) of rank %d holds 0x%08x, expected 0x%08x"
                        % (stride, k % case.size[0], k // case.size[0], int(owner.reshape(-1)[k]), int(got[k]), int(want[k])))
    if top - 1 > 0:                                                       # a stride below a rank's count is rejected, nothing is written
        gathered = upload(np.full(world * top, PADDING, np.uint32))
        target = upload(np.full(npix, TARGET, np.uint32))
        with pytest.raises(lib.FovptError) as e:
            r.gather_unpack(gathered.data_ptr(), top - 1, target.data_ptr())
        assert e.value.code == E_INVALID and "stride %d is smaller" % (top - 1) in str(e.value)
        r.synchronize()
        assert (words(target) == TARGET).all()


# ---- the plan cache --------------------------------------------------------------------------------------------------------------------
BASE = dict(size=(96, 64), gaze=(40, 30), radii=(6, 14), uniform=False, world=5, tile=(8, 4))
CHANGES = [("width", dict(size=(100, 64))), ("height", dict(size=(96, 68))), ("gaze x", dict(gaze=(41, 30))), ("gaze y", dict(gaze=(40, 31))),
           ("r_inner", dict(radii=(7, 14))), ("r_outer", dict(radii=(6, 15))), ("uniform", dict(uniform=True, radii=None)),
           ("world", dict(world=4)), ("tile_w", dict(tile=(5, 4))), ("tile_h", dict(tile=(8, 3)))]


def test_plan_cache_follows_every_ingredient(r):
    """One context; one ingredient of the plan changes at a time and changes back.  A key that missed one would serve the plan of
    the frame before."""
    configure(r, **BASE)
    base_lists, base_counts = check_plan(r, **BASE)
    for what, change in CHANGES:
        p = dict(BASE, **change)
        lists, counts = restated_for(**p)[1:]
        assert len(lists) != len(base_lists) or any(not np.array_equal(a, b) for a, b in zip(lists, base_lists)), what   # (a change that shows)
        configure(r, **p)
        try:
            check_plan(r, **p)
            configure(r, **BASE)
            check_plan(r, **BASE)
        except BaseException as e:
            raise AssertionError("after a change of %s: %s" % (what, e)) from e


def test_plan_ignores_what_is_no_ingredient(r):
    """rank, the spp fields, max_depth, subframe_index and the camera leave the plan as it was."""
    cfg = configure(r, **BASE)
    base_lists, base_counts = check_plan(r, **BASE)

    def same():
        assert r.gather_plan() == base_counts
        assert_packs_are_the_plan(iota_packs(r, *BASE["size"], base_counts), base_lists, BASE["size"][0])

    for rank in (1, 2):
        set_rank(r, rank)
        same()
    for field, value in (("spp_periphery", 3), ("spp_middle", 5), ("spp_fovea", 7), ("spp_uniform", 2), ("max_depth", 9)):
        c = cfg.copy()
        setattr(c, field, value)
        r.config = c
        same()
    r.config = cfg
    r.launchParams.frame.subframe_index = 17
    same()
    r.launchParams.frame.subframe_index = 0
    r.setCamera(renderer.Camera((0.3, 1.1, 2.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 50.0))
    same()


# ---- the plan against the renderer's own ownership -------------------------------------------------------------------------------
def test_plan_is_what_each_rank_renders():
    """k_generate_owned and k_resolve at a tile that is not the default: the pixels a rank's frame holds after fovpt_render (alpha
    255; another rank's pixels are zeroed, tests/resolve_ref.py) are that rank's plan list."""
    size, gaze, radii, world, tile = (64, 48), (30, 22), (5, 12), 3, (5, 3)
    owner, lists, counts = restated_for(size, gaze, radii, False, world, tile)
    assert min(counts) > 0
    cfg = cfg_foveated(radii[0], radii[1], (1, 1, 1))
    cfg.world, cfg.tile_w, cfg.tile_h = world, tile[0], tile[1]
    ctx = make_gpu(scenes.cornell_box(), scenes.ambient_probe(64, 32, 2.0), scenes.CORNELL_CAMERA, size, cfg, gaze=gaze)
    try:
        for rank in range(world):
            set_rank(ctx, rank)
            ctx.render()
            px = ctx.downloadPixels().reshape(-1)
            assert np.array_equal(np.flatnonzero(px), lists[rank]), rank
            assert ((px[lists[rank]] >> 24) == 255).all(), rank
            assert ctx.gather_plan() == counts
    finally:
        ctx.close()


# ---- rejections --------------------------------------------------------------------------------------------------------------------------
def test_rejections():
    ctx = renderer.SampleRenderer(scenes.cornell_box())
    L = ctx._L
    try:
        ctx.resize((16, 8))
        a, b = upload(np.zeros(16 * 8 + TAIL, np.uint32)), upload(np.zeros(16 * 8 + TAIL, np.uint32))

        def last():
            return L.fovpt_last_error(ctx._ctx).decode()

        # pack and unpack before any plan
        assert L.fovpt_gather_pack(ctx._ctx, a.data_ptr(), b.data_ptr()) == E_INVALID and "without a plan" in last() and "pack" in last()
        assert L.fovpt_gather_unpack(ctx._ctx, a.data_ptr(), 128, b.data_ptr()) == E_INVALID and "without a plan" in last() and "unpack" in last()
        # fewer counts than ranks
        cfg = configure(ctx, (16, 8), (8, 4), None, True, 4, None)
        counts = (C.c_uint32 * 4)(*[0xffffffff] * 4)
        assert L.fovpt_gather_plan(ctx._ctx, C.byref(ctx.launchParams), counts, 3) == E_INVALID
        assert "counts_out holds 3 entries, world is 4" in last()
        assert list(counts) == [0xffffffff] * 4
        assert L.fovpt_gather_pack(ctx._ctx, a.data_ptr(), b.data_ptr()) == E_INVALID          # (a refused plan is no plan)
        # more ranks than a plan holds
        cfg.world = 65
        try:
            ctx.config = cfg
        except lib.FovptError as e:                                       # (refused already by fovpt_set_config: as good)
            assert e.code == E_INVALID
        else:
            counts = (C.c_uint32 * 65)()
            assert L.fovpt_gather_plan(ctx._ctx, C.byref(ctx.launchParams), counts, 65) == E_INVALID
            assert "64 ranks" in last() and "65" in last()
        # null arguments
        assert L.fovpt_gather_plan(None, C.byref(ctx.launchParams), None, 0) == E_INVALID
        assert L.fovpt_gather_plan(ctx._ctx, None, None, 0) == E_INVALID
        assert L.fovpt_gather_pack(ctx._ctx, None, b.data_ptr()) == E_INVALID and L.fovpt_gather_unpack(ctx._ctx, a.data_ptr(), 128, None) == E_INVALID
        # and the context still plans: counts_out may be null
        configure(ctx, (16, 8), (8, 4), None, True, 4, None)
        assert L.fovpt_gather_plan(ctx._ctx, C.byref(ctx.launchParams), None, 0) == 0
        assert ctx.gather_plan() == restated_for((16, 8), (8, 4), None, True, 4, None)[2]
        ctx.synchronize()
        assert not words(a).any() and not words(b).any()
    finally:
        ctx.close()
