"""Checks of fovpt_temporal on the GPU against tests/temporal_ref.py (Checker, tcfg, cap_map) and the quality measurement over
the atrium: used by the temporal, temporal-motion, post and warp-motion tests.  General helpers are in tests/gpu_common.py.

Every expectation is computed from the GPU's own inputs: the input frame, the G-buffers fovpt_gbuffer builds at the current
camera (and kept from the previous step), and the history the previous step wrote.  The frame's description -- size, gaze,
radii, FOV_OFF flag, camera -- is r.launchParams and r.config as they were at render time: the callers leave them so until
the step is checked."""
import numpy as np

import reconstruct_ref as rr
import temporal_ref as tr
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer, scenes

from gpu_common import bits, camera, with_entries, writer_fills


def tcfg(d=None):
    """fovpt_temporal_defaults with the entries of d replaced."""
    c = abi.TemporalConfig()
    lib.check(None, lib.load().fovpt_temporal_defaults(c))
    return with_entries(c, d)


def cap_map(r, d=None):
    fill, uniform = writer_fills(r)
    return tr.caps(fill, uniform, d)


class Checker:
    """Follows one renderer's temporal steps: after each, out_color, out_rgba and the history equal the restatement on the
    GPU's inputs (prev: the GPU's previous G-buffer and history), and the restatement chained on its own outputs (chain)."""

    def __init__(self, oracle, r, d=None):
        self.oracle, self.r, self.d = oracle, r, dict(d or {})
        self.prev = self.chain = None

    def reset(self):
        self.prev = self.chain = None

    def step(self, inp=None, in_ptr=None, out=None):
        """r.temporal(d, in_ptr, out) on the frame just rendered.  inp: the input frame as numpy (None: the accum buffer, read
        before the call); out: None (the renderer's buffers) or (colour, rgba) device pointers.  -> (colour, history, cap)"""
        r = self.r
        inp = r.downloadAccum() if inp is None else inp
        r.temporal(tcfg(self.d), in_ptr, *(out or (None, None)))
        f = r.launchParams.frame
        shape = (f.size.y, f.size.x)
        if out is None:
            got_c, got_px = r.downloadTemporalColor(), r.downloadTemporalPixels()
        else:
            got_c = r.download(out[0], np.empty(shape + (4,), np.float32))
            got_px = r.download(out[1], np.empty(shape, np.uint32))
        got_h = r.downloadTemporalHistory()
        gb = r.downloadGBuffer()
        cam, cap = camera(r), cap_map(r, self.d)
        want_c, want_h = tr.step(inp, gb, cap, cam, self.prev, self.d)
        assert np.array_equal(bits(got_c), bits(want_c))
        assert np.array_equal(bits(got_h), bits(want_h))
        assert np.array_equal(got_px, self.oracle.make_color(want_c[..., :3].reshape(-1, 3)).reshape(shape))
        chain_c, chain_h = tr.step(inp, gb, cap, cam, self.chain, self.d)
        assert np.array_equal(bits(chain_c), bits(want_c)) and np.array_equal(bits(chain_h), bits(want_h))
        self.prev = dict(gb=gb, cam=cam, history=got_h)
        self.chain = dict(gb=gb, cam=cam, history=chain_h)
        return got_c, got_h, cap


# ---- the quality measurement of the test suite and tools/temporal_perf.py --sweep ---------------------------------------
def _atrium(size, cfg):
    cfg.write_guides = 1
    cam = scenes.ATRIUM_CAMERA
    r = renderer.SampleRenderer(scenes.atrium(8000))
    r.resize(size)
    r.setCamera(renderer.Camera(cam["eye"], cam["lookat"], cam["up"], cam["fovy"], size[0] / float(size[1])))
    r.setProbe(renderer.ProbeData(scenes.ambient_probe(96, 54, 2.5)).BuildCDF())
    r.config = cfg
    r.launchParams.frame.c.x, r.launchParams.frame.c.y = size[0] // 2, size[1] // 2
    return r


def _path_view(r, k, size):
    """Frame k of the slow camera path: the eye drifts about 7 units a frame, the look-at point 5."""
    cam = scenes.ATRIUM_CAMERA
    eye = (cam["eye"][0] + 6.0 * k, cam["eye"][1] + 1.0 * k, cam["eye"][2] + 4.0 * k)
    look = (cam["lookat"][0], cam["lookat"][1], cam["lookat"][2] - 5.0 * k)
    r.setCamera(renderer.Camera(eye, look, cam["up"], cam["fovy"], size[0] / float(size[1])))


def quality_truth(size=(384, 216), frames=12):
    """The GPU's own 256-spp FOV_OFF frame at the path's last camera."""
    c = abi.Config.reference_default()
    c.uniform, c.spp_uniform = 1, 256
    t = _atrium(size, c)
    _path_view(t, frames - 1, size)
    t.render()
    truth = t.downloadAccum()
    t.close()
    return truth


def quality_run(size=(384, 216), frames=12, configs=(None,), truth=None):
    """384 x 216 atrium, radii 30 / 90, spp (1, 2, 8), gaze at the centre: render -> reconstruct -> temporal over the slow
    camera path, for each temporal config (a dict of overrides) in turn on a fresh renderer.  -> one dict per config
    {level: (RMSE reconstruct only, RMSE with temporal)} on the last frame, periphery / middle / fovea."""
    truth = quality_truth(size, frames) if truth is None else truth
    rmse = lambda img, m: float(np.sqrt(((img[..., :3].astype(np.float64) - truth[..., :3]) ** 2)[m].mean()))
    out = []
    for d in configs:
        c = abi.Config.reference_default()
        c.r_inner, c.r_outer = 30, 90
        c.spp_periphery, c.spp_middle, c.spp_fovea = 1, 2, 8
        r = _atrium(size, c)
        dd = tcfg(d)
        for k in range(frames):
            _path_view(r, k, size)
            r.render()
            r.reconstruct()
            r.temporal(dd, r.reconstruct_buffers()[0])
        rec, tem = r.downloadReconstructedColor(), r.downloadTemporalColor()
        f = r.launchParams.frame
        fill = rr.writers(size[0], size[1], (f.c.x, f.c.y), 30, 90, 0)[0]
        r.close()
        out.append({name: (rmse(rec, fill == fl), rmse(tem, fill == fl)) for name, fl in (("periphery", 4), ("middle", 2), ("fovea", 1))})
    return out
