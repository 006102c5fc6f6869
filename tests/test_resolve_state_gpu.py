"""k_resolve on chosen path states (fovpt_debug_resolve): the production kernel, launched as a job launches it on the frame a
render() or a launch() of the case's parameters would resolve, against the painting restatement of tests/resolve_ref.py --
accum, rgba8 and the guide buffers compared as bits, pixel by pixel; pixels nobody writes must keep what they held, and the
state set's queue counters must come back zero.  tests/test_resolve_state_cpu.py ties the restatement to the oracle and shows
what each case of tests/resolve_cases.py reaches."""
import ctypes as C

import numpy as np
import pytest

import resolve_cases as rc
from common import cfg_uniform, make_gpu
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer, scenes

pytestmark = pytest.mark.gpu

BUFFERS = ("accum", "frame", "color", "normal", "albedo")


@pytest.fixture(scope="module")
def r():
    rr_ = renderer.SampleRenderer(scenes.cornell_box())
    yield rr_
    rr_.close()


def _install(r, case):
    """The case's configuration and launch parameters on the renderer, with frame buffers of the test's own holding the
    case's prefill -> the device tensors."""
    import torch
    r.config = case.config()
    case.set_params(r.launchParams)
    dev = {k: torch.from_numpy(v).cuda() for k, v in case.prefill().items()}
    torch.cuda.synchronize()
    f = r.launchParams.frame
    f.accum_buffer, f.frame_buffer = dev["accum"].data_ptr(), dev["frame"].data_ptr()
    f.color_buffer, f.normal_buffer, f.albedo_buffer = dev["color"].data_ptr(), dev["normal"].data_ptr(), dev["albedo"].data_ptr()
    return dev


def _run(r, case, st):
    dev = _install(r, case)
    left = r.debug_resolve(st["state"], st["cells"], st["alpha"], st["backplate"], guide_n=st["guide_n"] if case.guides else None,
                           guide_a=st["guide_a"] if case.guides else None, render=case.render is not None,
                           width=case.grid()[0], height=case.grid()[1])
    return {k: v.cpu().numpy() for k, v in dev.items()}, left


@pytest.mark.parametrize("case", rc.cases(), ids=lambda c: c.name)
def test_resolve(oracle, r, case):
    st = case.state()
    want, last = case.expected(oracle.make_color, st)
    passes, slots, launches = case.passes()
    _install(r, case)
    table = r.debug_resolve_passes(case.render is not None, *case.grid())
    assert [(p.gw, p.rows, p.spp, p.slot_base, p.launch_base) for p in table] == [(P.gw, P.gh, P.spp, P.slot_base, P.launch_base) for P in passes]
    got, left = _run(r, case, st)
    print(case.name, "slots", slots, "pixels written", int((last >= 0).sum()), "of", last.size, "counter words left", left)
    for k in BUFFERS:
        bad = got[k].view(np.uint32) != want[k].view(np.uint32)
        bad = bad.any(axis=-1) if bad.ndim == 3 else bad
        idx = np.argwhere(bad)
        assert idx.size == 0, (case.name, k, len(idx), "first (y, x):", idx[:4].tolist(), "pass of the last writer:", last[bad][:4].tolist(),
                               got[k][bad][:2], want[k][bad][:2])
    assert np.isfinite(got["accum"][last >= 0]).all()
    assert left == 0, "the resolve left %d queue-counter words non-zero" % left


def test_the_set_is_left_as_a_job_expects_it(oracle):
    """A frame rendered after the hook has used a state set is the frame rendered before."""
    size = (32, 32)
    r = make_gpu(scenes.cornell_box(), scenes.sky_probe(32, 16), scenes.CORNELL_CAMERA, size, cfg_uniform(1, 4))
    try:
        frames = []
        for k in range(4):
            r.launchParams.frame.subframe_index = 0
            r.render()
            frames.append((r.downloadAccum(), r.downloadPixels()))
            if k < 3:
                # (a uniform 32 x 32 frame, like the render's: resolved into the renderer's own buffers, then rendered over)
                case = rc.Case("hook", size, render=dict(uniform=1), seed=3 + k)
                st = case.state()
                assert r.debug_resolve(st["state"], st["cells"], st["alpha"], st["backplate"]) == 0
                assert not np.array_equal(r.downloadPixels(), frames[0][1])
        for a, p in frames[1:]:
            assert np.array_equal(a.view(np.uint32), frames[0][0].view(np.uint32)) and np.array_equal(p, frames[0][1])
    finally:
        r.close()


def test_the_hook_refuses_bad_arguments(r):
    L, ctx = r._L, r._ctx
    E_INVALID, E_NO_FRAME = -1, -5
    case = rc.cases()[1]
    _keep = _install(r, case)
    st = case.state()
    passes, n, left = (abi.DebugPass * 3)(), C.c_int(0), C.c_uint32(0)
    lp = r.launchParams
    args = lambda: (st["state"].ctypes.data, st["cells"].ctypes.data, st["alpha"].ctypes.data, None, None, st["backplate"].ctypes.data, C.byref(left))
    assert L.fovpt_debug_resolve(None, C.byref(lp), 1, 0, 0, passes, C.byref(n), *args()) == E_INVALID
    assert L.fovpt_debug_resolve(ctx, None, 1, 0, 0, passes, C.byref(n), *args()) == E_INVALID
    assert L.fovpt_debug_resolve(ctx, C.byref(lp), 1, 0, 0, None, C.byref(n), *args()) == E_INVALID
    assert L.fovpt_debug_resolve(ctx, C.byref(lp), 1, 0, 0, passes, C.byref(n), st["state"].ctypes.data, None, st["alpha"].ctypes.data, None, None,
                                 st["backplate"].ctypes.data, C.byref(left)) == E_INVALID
    bare = lp.copy()
    bare.frame.accum_buffer = None
    assert L.fovpt_debug_resolve(ctx, C.byref(bare), 1, 0, 0, passes, C.byref(n), *args()) == E_NO_FRAME
    zero = lp.copy()
    zero.samples_per_launch = 0
    assert L.fovpt_debug_resolve(ctx, C.byref(zero), 0, 4, 4, passes, C.byref(n), *args()) == E_INVALID
    cfg = case.config()
    cfg.write_guides = 1                                    # guides wanted, none given
    r.config = cfg
    assert L.fovpt_debug_resolve(ctx, C.byref(lp), 1, 0, 0, passes, C.byref(n), *args()) == E_INVALID
    r.config = case.config()
    # the parameters were not changed by any of this, and a good call still works
    assert lp.frame.subframe_index == case.subframe
    assert L.fovpt_debug_resolve(ctx, C.byref(lp), 1, 0, 0, passes, C.byref(n), *args()) == 0 and n.value == 1 and left.value == 0
