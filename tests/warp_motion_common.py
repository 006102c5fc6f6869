"""Checks of fovpt_warp_motion on the GPU against tests/warp_motion_ref.py (Intervals, mcfg, frame_data, check): used by
test_warp_motion_gpu.py, test_warp_motion_fuzz_gpu.py and the application fuzz.  General helpers are in tests/gpu_common.py.

Every expectation is computed from the GPU's own data -- the G-buffer and hit records fovpt_gbuffer builds at the rendered camera
(it traces the same rays), the inputs -- and from the vertex arrays the test itself uploaded, in MotionChecker's bookkeeping."""
import numpy as np

import warp_motion_ref as wm
import warp_ref as wr
from fovpathtracing_optixcodelatest_amd import renderer

from gpu_common import bits, camera, device_images, host_view, with_entries
from temporal_motion_common import MotionChecker, download_hits
from test_warp_gpu import counts_of

STEPS = ("temporal", "temporal_motion", "post")


class Intervals(MotionChecker):
    """MotionChecker's bookkeeping of updates, for the warp: end_interval() runs a temporal step through one of the three calls
    without checking it (their own tests do) and keeps what the interval it ended looked like -- self.last: the dict motion()
    made just before the step, or None where the step knew nothing of the interval's motion (an update ran before the
    tracking of previous positions was on)."""

    def __init__(self, r):
        super().__init__(None, r, None)
        self.last = None
        self.stepped = False                                 # a step whose previous positions fovpt_warp_motion may use

    def end_interval(self, how="temporal_motion"):
        assert how in STEPS
        m = self.motion()
        getattr(self.r, how)()
        if how != "temporal":
            self.tracking = True
        self.last = None if self.untracked else m
        self.untracked = False
        self.vtx_step = self.vtx.copy()
        self.moved[:] = False
        self.stepped = True

    def moved_last(self):
        return self.last is not None and bool(self.last["moved"].any())


def mcfg(**d):
    return with_entries(renderer.SampleRenderer.warp_motion_defaults(), d)


def frame_data(r):
    """(G-buffer, (u, v) of the hit records) of the rendered camera, traced now: the camera must be the rendered frame's."""
    gb = r.downloadGBuffer()
    return gb, download_hits(r)[..., 1:3]


def check(r, ck, to, want_cam, gb, uv, color, rgba, advance, radius, images, gbuffer=None, label=None):
    """One fovpt_warp_motion into caller's buffers against the restatement: every pixel of every enabled output, the map and the
    four counts; an image that is not enabled keeps its bytes.  -> the restatement's output."""
    f = r.launchParams.frame
    size = (f.size.x, f.size.y)
    oc, op, om = device_images(size, 16, 4, 4)
    r.warp_motion(to, mcfg(images=images, fill_radius=radius, advance=advance), gbuffer, None, None, oc.data_ptr(), op.data_ptr(), om.data_ptr())
    got_counts = counts_of(r)
    want = wm.warp(gb, uv, ck.last, camera(r), want_cam, dict(images=images, fill_radius=radius, advance=advance), color, rgba)
    assert np.array_equal(host_view(om, "map"), want["map"]), label
    assert got_counts == want["counts"] and sum(got_counts[1:]) == size[0] * size[1], (label, got_counts, want["counts"])
    if images & wr.COLOR:
        assert np.array_equal(bits(host_view(oc, "color")), bits(want["color"])), label
    else:
        assert (oc.cpu().numpy() == 0x5a).all(), label
    if images & wr.RGBA:
        assert np.array_equal(host_view(op, "rgba"), want["rgba"]), label
    else:
        assert (op.cpu().numpy() == 0x5a).all(), label
    return want
