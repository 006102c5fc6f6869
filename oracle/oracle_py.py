"""ctypes access to the CPU oracle (oracle/libfovpt_oracle.so).

TEST INFRASTRUCTURE: imported only by tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg.  The product package never imports this module.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from fovpathtracing_optixcodelatest_amd import abi
from fovpathtracing_optixcodelatest_amd.scenes import pack_model

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libfovpt_oracle.so")


def build(force=False):
    src = os.path.join(_HERE, "fovpt_oracle.cpp")
    if force or not os.path.exists(_SO) or os.path.getmtime(_SO) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", _HERE, "-s"] + (["-B"] if force else []))
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            build()
        L = C.CDLL(_SO)
        L.orc_scene_create.restype = C.c_void_p
        L.orc_scene_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.orc_scene_destroy.argtypes = [C.c_void_p]
        L.orc_scene_num_triangles.restype = C.c_uint64
        L.orc_scene_num_triangles.argtypes = [C.c_void_p]
        L.orc_launch.argtypes = [C.c_void_p, C.POINTER(abi.LaunchParams), C.c_uint32, C.c_uint32,
                                 C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.orc_render.argtypes = [C.c_void_p, C.POINTER(abi.LaunchParams), C.POINTER(abi.Config),
                                 C.c_int, C.c_int, C.c_void_p]
        L.orc_tea4.restype = C.c_uint32
        L.orc_tea4.argtypes = [C.c_uint32, C.c_uint32]
        L.orc_trace.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.orc_math.argtypes = [C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.orc_lib_counts.argtypes = [C.c_void_p, C.c_int]
        L.orc_shade_hit.argtypes = [C.c_void_p, C.POINTER(abi.Probe), C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
        L.orc_record_samples.restype = C.c_uint64
        L.orc_record_samples.argtypes = [C.c_void_p, C.c_uint64]
        L.orc_camera_uvw.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.orc_camera_rays.argtypes = [C.POINTER(abi.LaunchParams), C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 7
        _lib = L
    return _lib


def set_lib_counting(on: bool):
    """Counts.lib_* need one BSDF evaluation more than the reference does on occluded shadow rays; the timed CPU
    baseline turns the counting off (the counts of such a run are meaningless)."""
    lib().orc_set_lib_counting(1 if on else 0)


def set_math_mode(detmath: bool):
    lib().orc_set_math_mode(1 if detmath else 0)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class OracleScene:
    def __init__(self, model):
        md, n, td, nt, keep = pack_model(model)
        self._h = lib().orc_scene_create(C.cast(md, C.c_void_p), n, C.cast(td, C.c_void_p), nt)
        self.num_triangles = lib().orc_scene_num_triangles(self._h)

    def __del__(self):
        if getattr(self, "_h", None):
            lib().orc_scene_destroy(self._h)
            self._h = None

    def trace(self, origins, dirs, brute=False):
        o = np.ascontiguousarray(origins, np.float32)
        d = np.ascontiguousarray(dirs, np.float32)
        n = o.shape[0]
        prim = np.empty(n, np.uint32)
        tuv = np.empty((n, 3), np.float32)
        occ = np.empty(n, np.uint8)
        lib().orc_trace(self._h, n, _p(o), _p(d), int(brute), _p(prim), _p(tuv), _p(occ))
        return prim, tuv, occ


def build_cdf(data):
    """ProbeData::BuildCDF restatement.  data: (H,W,4) float32 -> pdfX, cdfX, pdfY, cdfY"""
    data = np.ascontiguousarray(data, np.float32)
    h, w = data.shape[:2]
    pdfx = np.empty((h, w), np.float32)
    cdfx = np.empty((h, w), np.float32)
    pdfy = np.empty(h, np.float32)
    cdfy = np.empty(h, np.float32)
    lib().orc_build_cdf(w, h, _p(data), _p(pdfx), _p(cdfx), _p(pdfy), _p(cdfy))
    return pdfx, cdfx, pdfy, cdfy


class HostProbe:
    """fovpt_probe with HOST pointers, for the oracle."""

    def __init__(self, data, cdf=None):
        self.data = np.ascontiguousarray(data, np.float32)
        self.pdfx, self.cdfx, self.pdfy, self.cdfy = cdf if cdf is not None else build_cdf(self.data)
        p = abi.Probe()
        p.height, p.width = self.data.shape[:2]
        p.data = self.data.ctypes.data
        p.pdfValuesX, p.cdfValuesX = self.pdfx.ctypes.data, self.cdfx.ctypes.data
        p.pdfValuesY, p.cdfValuesY = self.pdfy.ctypes.data, self.cdfy.ctypes.data
        self.struct = p


def camera_uvw(eye, lookat, up, fovy, aspect):
    e, l, u = (np.asarray(x, np.float32) for x in (eye, lookat, up))
    U, V, W = np.empty(3, np.float32), np.empty(3, np.float32), np.empty(3, np.float32)
    lib().orc_camera_uvw(_p(e), _p(l), _p(u), fovy, aspect, _p(U), _p(V), _p(W))
    return U, V, W


class OracleFrame:
    """Host frame buffers + LaunchParams for the oracle; mirrors what SampleRenderer holds."""

    def __init__(self, width, height, probe: HostProbe, camera: dict, gaze=None, subframe_index=0):
        self.w, self.h = width, height
        self.accum = np.zeros((height, width, 4), np.float32)
        self.frame = np.zeros((height, width), np.uint32)
        self.normal = np.zeros((height, width, 4), np.float32)
        self.color = np.zeros((height, width, 4), np.float32)
        self.albedo = np.zeros((height, width, 4), np.float32)
        self.probe = probe
        lp = abi.LaunchParams()
        lp.frame.accum_buffer = self.accum.ctypes.data
        lp.frame.frame_buffer = self.frame.ctypes.data
        lp.frame.normal_buffer = self.normal.ctypes.data
        lp.frame.color_buffer = self.color.ctypes.data
        lp.frame.albedo_buffer = self.albedo.ctypes.data
        lp.frame.size.x, lp.frame.size.y = width, height
        lp.frame.subframe_index = subframe_index
        gx, gy = gaze if gaze is not None else (width // 2, height // 2)
        lp.frame.c.x, lp.frame.c.y = gx, gy
        U, V, W = camera_uvw(camera["eye"], camera["lookat"], camera["up"], camera["fovy"], width / float(height))
        lp.camera.eye.set(camera["eye"])
        lp.camera.U.set(U)
        lp.camera.V.set(V)
        lp.camera.W.set(W)
        lp.probe = probe.struct
        self.lp = lp


class Counts(tuple):
    """(radiance_rays, shadow_rays, paths) as the REFERENCE traces them, plus .lib_radiance / .lib_shadow: the rays
    libfovpt traces for the same frame (it skips the reference's discarded last segment and shadow rays that cannot
    change a bit of the image; fovpt_oracle.cpp, g_lib_radiance).  The library's device counters must equal them."""
    lib_radiance = 0
    lib_shadow = 0


def _counts(cnt):
    lc = np.zeros(2, np.uint64)
    lib().orc_lib_counts(_p(lc), 1)
    c = Counts(int(x) for x in cnt)
    c.lib_radiance, c.lib_shadow = int(lc[0]), int(lc[1])
    return c


def render(scene: OracleScene, frame: OracleFrame, cfg: abi.Config, brute=False, nthreads=None):
    """SampleRenderer::render() on the CPU.  Returns Counts(radiance_rays, shadow_rays, paths)."""
    if nthreads is None:
        nthreads = os.cpu_count() or 1
    cnt = np.zeros(3, np.uint64)
    lib().orc_lib_counts(None, 1)
    rc = lib().orc_render(scene._h, C.byref(frame.lp), C.byref(cfg), int(brute), int(nthreads), _p(cnt))
    if rc != 0:
        raise RuntimeError("orc_render failed: %d" % rc)
    return _counts(cnt)


def launch(scene: OracleScene, frame: OracleFrame, width, height, max_depth=4, accumulate=0, brute=False, nthreads=None):
    if nthreads is None:
        nthreads = os.cpu_count() or 1
    cnt = np.zeros(3, np.uint64)
    lib().orc_lib_counts(None, 1)
    rc = lib().orc_launch(scene._h, C.byref(frame.lp), width, height, max_depth, accumulate, int(brute), int(nthreads), _p(cnt))
    if rc != 0:
        raise RuntimeError("orc_launch failed: %d" % rc)
    return _counts(cnt)


def shade_hit(scene: OracleScene, probe: "HostProbe", max_depth, options, origin, dir4, prim, tuv, rng3, thr4, occluded):
    """traceRadiance from just behind trace_closest on given hits, the outcome of the occlusion test given -> dict of the
    RadiancePRD afterwards (flags, depth, radiance, alpha, origin, direction, bsdfPdf, thr, eta, rng (n, 2) uint32, normal, albedo,
    sky_added, rr_kill) and kind (0 miss, 1 catcher pass-through, 2 shaded, 3 shaded on a catcher), P, wi."""
    o = np.ascontiguousarray(origin, np.float32).reshape(-1, 3)
    n = o.shape[0]
    d = np.ascontiguousarray(dir4, np.float32).reshape(n, 4)
    prim = np.ascontiguousarray(prim, np.uint32).reshape(n)
    tuv = np.ascontiguousarray(tuv, np.float32).reshape(n, 3)
    rng3 = np.ascontiguousarray(rng3, np.uint32).reshape(n, 3)
    thr4 = np.ascontiguousarray(thr4, np.float32).reshape(n, 4)
    out = np.empty((n, lib().orc_shade_hit_row_floats()), np.float32)
    rc = lib().orc_shade_hit(scene._h, C.byref(probe.struct), int(max_depth), int(options), n, _p(o), _p(d), _p(prim), _p(tuv), _p(rng3), _p(thr4),
                             1 if occluded else 0, _p(out))
    if rc != 0:
        raise RuntimeError("orc_shade_hit failed: %d" % rc)
    ints = lambda k: out[:, k].astype(np.int64)
    return dict(kind=ints(0), flags=ints(1), depth=ints(2), radiance=out[:, 3:6].copy(), alpha=out[:, 6:9].copy(), origin=out[:, 9:12].copy(),
                direction=out[:, 12:15].copy(), bsdfPdf=out[:, 15].copy(), thr=out[:, 16:19].copy(), eta=out[:, 19].copy(),
                rng=out[:, 20:22].copy().view(np.uint32), normal=out[:, 22:25].copy(), albedo=out[:, 25:28].copy(),
                sky_added=ints(28), rr_kill=ints(29), P=out[:, 30:33].copy(), wi=out[:, 33:36].copy())


class SampleRecording:
    """with SampleRecording(capacity) as rec: render(...) / launch(...) -- afterwards rec.rows holds the per-sample terms of those
    launches, one row per traced sample in the order they ran: dict(launch, lx, ly, sample, nterm, alpha, normal, albedo,
    backplate, terms): `terms` (n, 32, 3) are what the sample added to directLight (the first) and indirectLight, in order."""

    def __init__(self, capacity):
        self._buf = np.zeros((capacity, lib().orc_sample_row_floats()), np.float32)
        self.rows = None

    def __enter__(self):
        lib().orc_record_samples(_p(self._buf), self._buf.shape[0])
        return self

    def __exit__(self, *exc):
        n = int(lib().orc_record_samples(None, 0))
        assert n <= self._buf.shape[0], "recorded %d samples, room for %d" % (n, self._buf.shape[0])
        b = self._buf[:n]
        ints = lambda k: b[:, k].astype(np.int64)
        self.rows = dict(launch=ints(0), lx=ints(1), ly=ints(2), sample=ints(3), nterm=ints(4), alpha=b[:, 5:8].copy(),
                         normal=b[:, 8:11].copy(), albedo=b[:, 11:14].copy(), backplate=b[:, 14:17].copy(),
                         terms=b[:, 17:].reshape(n, -1, 3).copy())
        return False


def math_op(op, a, b=None):
    a = np.ascontiguousarray(a, np.float32)
    bb = np.ascontiguousarray(b, np.float32) if b is not None else None
    out = np.empty_like(a)
    lib().orc_math(op, a.size, _p(a), _p(bb), _p(out))
    return out


# ---- unit-level entry points -----------------------------------------------------------------
def tea4(a, b):
    return int(lib().orc_tea4(a & 0xFFFFFFFF, b & 0xFFFFFFFF))


def lcg_stream(seed, n):
    u = np.empty(n, np.uint32)
    f = np.empty(n, np.float32)
    lib().orc_lcg_stream(C.c_uint32(seed & 0xFFFFFFFF), n, _p(u), _p(f))
    return u, f


def random_stream(seed, n):
    u = np.empty(n, np.uint32)
    f = np.empty(n, np.float32)
    s = seed if seed < 0x80000000 else seed - (1 << 32)
    lib().orc_random_stream(C.c_int(s), n, _p(u), _p(f))
    return u, f


def probe_sample(probe: "HostProbe", seed, n):
    d = np.empty((n, 3), np.float32)
    c = np.empty((n, 3), np.float32)
    p = np.empty(n, np.float32)
    lib().orc_probe_sample(C.byref(probe.struct), C.c_int(seed), n, _p(d), _p(c), _p(p))
    return d, c, p


def probe_sample_at(probe: "HostProbe", r12):
    """ProbeSample with its two random numbers given -> dict(row, col, dir, color, pdf)."""
    r = np.ascontiguousarray(r12, np.float32).reshape(-1, 2)
    n = r.shape[0]
    rc = np.empty((n, 2), np.int32)
    d = np.empty((n, 3), np.float32)
    c = np.empty((n, 3), np.float32)
    p = np.empty(n, np.float32)
    lib().orc_probe_sample_at(C.byref(probe.struct), n, _p(r), _p(rc), _p(d), _p(c), _p(p))
    return dict(row=rc[:, 0].copy(), col=rc[:, 1].copy(), dir=d, color=c, pdf=p)


def probe_eval(probe: "HostProbe", dirs):
    """ProbeDirToUV + ProbeEval (the backplate of a camera ray) -> dict(uv, texel)."""
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    uv = np.empty((d.shape[0], 2), np.float32)
    t = np.empty((d.shape[0], 4), np.float32)
    lib().orc_probe_eval_dir(C.byref(probe.struct), d.shape[0], _p(d), _p(uv), _p(t))
    return dict(uv=uv, texel=t)


CAMERA_VARIANTS = dict(reference=0, jy_first=1, random_late=2, signed_index=3, inner_edge_dead=4, skip_one_draw=5, first_backplate=6)


def camera_rays(lp, launch_indices, variant="reference"):
    """The head of the raygen program for the launch indices (n, 2) = (lx, ly) of ONE launch with the parameters lp (host probe):
    -> dict(alive (n,) bool, pixel (n, 2) uint32, range (n,) = the distance the ring test compared, rand (n, spp, 2) uint32 = Random(seed) of every sample, jitter (n, spp, 2),
    dir (n, spp, 3), backplate (n, 3) = the last sample's).  `variant` other than "reference": one deliberate deviation
    (CAMERA_VARIANTS), for tests that show their cases can tell."""
    li = np.ascontiguousarray(launch_indices, np.uint32).reshape(-1, 2)
    n, spp = li.shape[0], int(lp.samples_per_launch)
    alive, pixel, rng = np.zeros(n, np.uint8), np.zeros((n, 2), np.uint32), np.zeros(n, np.float32)
    rand, jitter = np.zeros((n, spp, 2), np.uint32), np.zeros((n, spp, 2), np.float32)
    d, bp = np.zeros((n, spp, 3), np.float32), np.zeros((n, 3), np.float32)
    rc = lib().orc_camera_rays(C.byref(lp), n, _p(li), CAMERA_VARIANTS[variant], _p(alive), _p(pixel), _p(rng), _p(rand), _p(jitter), _p(d), _p(bp))
    if rc != 0:
        raise RuntimeError("orc_camera_rays failed: %d" % rc)
    return dict(alive=alive.astype(bool), pixel=pixel, range=rng, rand=rand, jitter=jitter, dir=d, backplate=bp)


def probe_dir_to_uv(dirs):
    d = np.ascontiguousarray(dirs, np.float32)
    uv = np.empty((d.shape[0], 2), np.float32)
    lib().orc_probe_dir_to_uv(d.shape[0], _p(d), _p(uv))
    return uv


def bsdf_table(material, N, view, albedo, etaI, etaO, seeds):
    n = len(seeds)
    N, view, albedo = (np.ascontiguousarray(x, np.float32) for x in (N, view, albedo))
    etaI, etaO = np.ascontiguousarray(etaI, np.float32), np.ascontiguousarray(etaO, np.float32)
    seeds = np.ascontiguousarray(seeds, np.int32)
    light = np.empty((n, 3), np.float32)
    pdf = np.empty(n, np.float32)
    typ = np.empty(n, np.int32)
    ev = np.empty((n, 3), np.float32)
    pdf2 = np.empty(n, np.float32)
    rng = np.empty((n, 2), np.uint32)
    lib().orc_bsdf_table(C.byref(material), n, _p(N), _p(view), _p(albedo), _p(etaI), _p(etaO), _p(seeds),
                         _p(light), _p(pdf), _p(typ), _p(ev), _p(pdf2), _p(rng))
    return dict(light=light, pdf=pdf, type=typ, eval=ev, pdf_again=pdf2, rng_after=rng)


def bsdf_table_given(material, N, view, albedo, etaI, etaO, seeds, L_given):
    """bsdf_table's columns, and eval_given / pdf_given: BSDFEval and BSDFPdf at the light direction L_given of each row."""
    n = len(seeds)
    N, view, albedo, L_given = (np.ascontiguousarray(x, np.float32) for x in (N, view, albedo, L_given))
    etaI, etaO = np.ascontiguousarray(etaI, np.float32), np.ascontiguousarray(etaO, np.float32)
    seeds = np.ascontiguousarray(seeds, np.int32)
    light = np.empty((n, 3), np.float32)
    pdf = np.empty(n, np.float32)
    typ = np.empty(n, np.int32)
    ev = np.empty((n, 3), np.float32)
    pdf2 = np.empty(n, np.float32)
    rng = np.empty((n, 2), np.uint32)
    evg = np.empty((n, 3), np.float32)
    pdfg = np.empty(n, np.float32)
    lib().orc_bsdf_table_given(C.byref(material), n, _p(N), _p(view), _p(albedo), _p(etaI), _p(etaO), _p(seeds), _p(L_given),
                               _p(light), _p(pdf), _p(typ), _p(ev), _p(pdf2), _p(rng), _p(evg), _p(pdfg))
    return dict(light=light, pdf=pdf, type=typ, eval=ev, pdf_again=pdf2, rng_after=rng, eval_given=evg, pdf_given=pdfg)


def make_color(rgb):
    rgb = np.ascontiguousarray(rgb, np.float32)
    out = np.empty(rgb.shape[0], np.uint32)
    lib().orc_make_color(rgb.shape[0], _p(rgb), _p(out))
    return out


def tex2d(texture_u32, uv):
    px = np.ascontiguousarray(texture_u32, np.uint32)
    td = abi.TextureDesc()
    td.pixel, td.width, td.height = px.ctypes.data, px.shape[1], px.shape[0]
    uv = np.ascontiguousarray(uv, np.float32)
    out = np.empty((uv.shape[0], 4), np.float32)
    lib().orc_tex2d(C.byref(td), uv.shape[0], _p(uv), _p(out))
    return out
