"""Checks of fovpt_post on the GPU: used by test_post_gpu.py and test_post_fuzz_gpu.py.

Two kinds.  separate() makes the stage calls fovpt_post is defined as, on a twin context, and same() compares every output and
the state both leave behind bit for bit.  PostChecker compares a fovpt_post call with tests/post_ref.py on the GPU's own inputs,
the way temporal_motion_common.MotionChecker (whose bookkeeping of updates and tracking it inherits) gathers them."""
import numpy as np

import post_ref as po
import reconstruct_ref as rr
from fovpathtracing_optixcodelatest_amd import abi, lib

from gpu_common import bits, camera, with_entries
from postprocess_common import guides
from temporal_motion_common import MotionChecker, download_hits

D, R, T, M = po.DENOISE, po.RECONSTRUCT, po.TEMPORAL, po.MOTION


def pcfg(stages=None, denoise=None, reconstruct=None, temporal=None):
    """fovpt_post_defaults with the stages and the entries of the three dicts replaced."""
    c = abi.PostConfig()
    lib.check(None, lib.load().fovpt_post_defaults(c))
    if stages is not None:
        c.stages = stages
    for sub, d in ((c.denoise, denoise), (c.reconstruct, reconstruct), (c.temporal, temporal)):
        with_entries(sub, d)
    return c


def separate(r, pc, in_ptr=None, out=(None, None), out_motion=None):
    """The stage calls fovpt_post(pc, in_ptr, *out, out_motion) stands for: the last enabled one into `out`."""
    st, cur = pc.stages, in_ptr
    if st & D:
        r.denoise(pc.denoise, *(out if not st & (R | T) else (None, None)))
        cur = r.denoise_buffers()[0]
    if st & R:
        r.reconstruct(pc.reconstruct, cur, *(out if not st & T else (None, None)))
        cur = r.reconstruct_buffers()[0]
    if st & T:
        if st & M:
            r.temporal_motion(pc.temporal, cur, out[0], out[1], out_motion)
        else:
            r.temporal(pc.temporal, cur, *out)


def own_outputs(r, stages, post):
    """(colour, rgba8) of the context's own buffers of the chain's last stage: fovpt_post's (post) or the stage call's."""
    if post:
        return r.downloadPostColor(), r.downloadPostPixels()
    if stages & T:
        return r.downloadTemporalColor(), r.downloadTemporalPixels()
    if stages & R:
        return r.downloadReconstructedColor(), r.downloadReconstructedPixels()
    return r.downloadDenoisedColor(), r.downloadDenoisedPixels()


def same(a, b, stages, label, motion=True, stepped=None, a_posts=False):
    """Context a made the separate calls, b called fovpt_post: colour, rgba8, history, motion vectors and, where a stage follows
    the denoiser, the denoise buffers are equal bit for bit.  stepped: whether a temporal step has run on them (default: now);
    a_posts: context a called fovpt_post too."""
    (ca, pa), (cb, pb) = own_outputs(a, stages, a_posts), own_outputs(b, stages, True)
    assert np.array_equal(bits(ca), bits(cb)), label
    assert np.array_equal(pa, pb), label
    if stages & T if stepped is None else stepped:
        assert np.array_equal(bits(a.downloadTemporalHistory()), bits(b.downloadTemporalHistory())), label
    if stages & M and motion:
        assert np.array_equal(bits(a.downloadMotion()), bits(b.downloadMotion())), label
    if stages & D and stages & (R | T):
        assert np.array_equal(bits(a.downloadDenoisedColor()), bits(b.downloadDenoisedColor())), label
        assert np.array_equal(a.downloadDenoisedPixels(), b.downloadDenoisedPixels()), label
    return cb


def rendered_frame(r, inp, gb, uv, gaze=None):
    """post_ref's description of the frame r rendered last, from the GPU's own buffers (r.launchParams and r.config as they
    were at render time; gaze: the rendered frame's, where the caller has written the next one into r.launchParams since)."""
    f, cfg = r.launchParams.frame, r.config
    fill, pas, ax, ay = rr.writers(f.size.x, f.size.y, (f.c.x, f.c.y) if gaze is None else gaze, cfg.r_inner, cfg.r_outer, cfg.uniform)
    color, normal, albedo = guides(r) if cfg.write_guides else (None, None, None)
    return dict(inp=inp, color=color, normal=normal, albedo=albedo, gb=gb, uv=uv, fill=fill, pas=pas, ax=ax, ay=ay,
                uniform=cfg.uniform, cam=camera(r))


class PostChecker(MotionChecker):
    """Follows one renderer's updates (MotionChecker.update) and fovpt_post calls: after each, colour, rgba8, history, motion
    vectors and denoise buffers equal post_ref.post on the GPU's own inputs.  cfg: dict(denoise=, reconstruct=, temporal=)."""

    def __init__(self, oracle, r, stages=po.DEFAULT_STAGES, cfg=None):
        self.stages, self.cfg = stages, dict(cfg or {})
        self.gaze_rendered = None                                # set where r.launchParams no longer hold the rendered frame's gaze
        super().__init__(oracle, r, self.cfg.get("temporal"))

    def step(self, inp=None, in_ptr=None, out=None, with_motion=True, stages=None):
        """r.post() on the frame just rendered.  inp: the colour input as numpy (None: the accum buffer); out: None (the
        renderer's own buffers) or (colour, rgba) device pointers.  -> dict(color, history, motion, fill, gb, frame)"""
        r, st = self.r, self.stages if stages is None else stages
        inp = r.downloadAccum() if inp is None else inp
        mo_ptr = r.motion_buffer() if st & M and with_motion else None
        r.post(pcfg(st, **self.cfg), in_ptr, *(out or (None, None)), mo_ptr)
        f = r.launchParams.frame
        shape = (f.size.y, f.size.x)
        if out is None:
            got_c, got_px = r.downloadPostColor(), r.downloadPostPixels()
        else:
            got_c, got_px = r.download(out[0], np.empty(shape + (4,), np.float32)), r.download(out[1], np.empty(shape, np.uint32))
        got_h = r.downloadTemporalHistory() if st & T else None
        got_m = r.downloadMotion() if mo_ptr is not None else None
        got_d = r.downloadDenoisedColor() if st & D and st & (R | T) else None
        gb = r.downloadGBuffer()                                  # (the same rays as the step's own trace)
        uv = download_hits(r)[..., 1:3]
        frame = rendered_frame(r, inp, gb, uv, self.gaze_rendered)
        if st & M:
            if self.untracked:
                self.prev = None
            self.tracking = True
        if st & T:
            self.untracked = False
        want = po.post(st, frame, self.prev, self.cfg, self.motion() if st & M else None)
        assert np.array_equal(bits(got_c), bits(want["color"]))
        assert np.array_equal(got_px, self.oracle.make_color(want["color"][..., :3].reshape(-1, 3)).reshape(shape))
        if got_h is not None:
            assert np.array_equal(bits(got_h), bits(want["history"]))
        if got_m is not None:
            assert np.array_equal(bits(got_m), bits(want["motion"]))
        if got_d is not None:
            assert np.array_equal(bits(got_d), bits(want["denoised"]))
        if st & T:
            self.prev = dict(gb=gb, cam=frame["cam"], history=got_h)
            self.vtx_step = self.vtx.copy()
            self.moved[:] = False
        return dict(color=got_c, history=got_h, motion=got_m, fill=frame["fill"], gb=gb, frame=frame)
