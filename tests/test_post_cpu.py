"""fovpt_post without a GPU: its prototypes and struct in the header, the ctypes mirror and the C++ drop-in, null arguments, the
defaults, and properties of the definition, the composition of the stage restatements in tests/post_ref.py that the GPU chain
is checked against."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import header_layout
import post_ref as po
import reconstruct_ref as rr
import temporal_ref as tr
from fovpathtracing_optixcodelatest_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def so():
    lib.build()
    return lib.load()


def _args(hdr, name):
    m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
    assert m, "fovpt.h does not declare %s" % name
    return [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", a).strip()) for a in m.group(1).replace("\n", " ").split(",")]


def test_the_prototypes_agree_everywhere(so):
    hdr = open(os.path.join(ROOT, "include", "fovpt.h")).read()
    assert _args(hdr, "fovpt_post_defaults") == ["fovpt_post_config* out"]
    assert _args(hdr, "fovpt_post") == ["fovpt_ctx* ctx", "const fovpt_launch_params* lp", "const fovpt_post_config* pc",
                                        "const fovpt_float4* in_color", "fovpt_float4* out_color", "uint32_t* out_rgba",
                                        "fovpt_float4* out_motion"]
    assert _args(hdr, "fovpt_post_buffers") == ["fovpt_ctx* ctx", "fovpt_float4** color", "uint32_t** rgba"]
    for name, value in (("DENOISE", 1), ("RECONSTRUCT", 2), ("TEMPORAL", 4), ("MOTION", 8)):
        assert re.search(r"#define FOVPT_POST_%s\s+%d\b" % (name, value), hdr)
        assert getattr(abi, "POST_" + name) == getattr(po, name) == value
    vp = C.c_void_p
    assert list(so.fovpt_post_defaults.argtypes) == [C.POINTER(abi.PostConfig)]
    assert list(so.fovpt_post.argtypes) == [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.PostConfig), vp, vp, vp, vp]
    assert list(so.fovpt_post_buffers.argtypes) == [vp, C.POINTER(vp), C.POINTER(vp)]
    assert so.fovpt_post.restype == C.c_int
    names = subprocess.check_output(["nm", "-D", "--defined-only", lib.SO_PATH], text=True)
    for sym in ("fovpt_post_defaults", "fovpt_post", "fovpt_post_buffers"):
        assert re.search(r"\bT %s\b" % sym, names), sym
    shim = open(os.path.join(ROOT, "include", "SimplePathtracer.h")).read()
    call = re.search(r"fovpt_post\((.*?)\)\);", shim, re.S)
    assert call and len(call.group(1).replace("reinterpret_cast<const fovpt_launch_params*>(&launchParams)", "lp").split(",")) == 7
    assert "void post(" in shim and "void downloadPostPixels(" in shim


def test_the_dropin_header_compiles():
    src = '#include "SimplePathtracer.h"\nvoid f(SampleRenderer& s, fovpt_float4* m, uint32_t* h) { s.post(); fovpt_post_config pc; ' \
          'fovpt_post_defaults(&pc); pc.stages = FOVPT_POST_DENOISE | FOVPT_POST_RECONSTRUCT | FOVPT_POST_TEMPORAL | FOVPT_POST_MOTION; ' \
          's.post(pc); s.post(pc, nullptr, m); s.post(pc, m); s.downloadPostPixels(h); }\n'
    header_layout.syntax_check(src)


def test_the_struct_mirror_matches_the_header():
    names = [f[0] for f in abi.PostConfig._fields_]
    got = header_layout.layout("fovpt_post_config", abi.PostConfig)
    assert got[0] == C.sizeof(abi.PostConfig) == 112
    assert got[1:] == [getattr(abi.PostConfig, n).offset for n in names]
    assert (abi.PostConfig.denoise.offset, abi.PostConfig.reconstruct.offset, abi.PostConfig.temporal.offset) == (16, 48, 80)


def test_post_defaults_are_the_stage_defaults(so):
    p = abi.PostConfig()
    C.memset(C.byref(p), 0xff, C.sizeof(p))
    assert so.fovpt_post_defaults(C.byref(p)) == 0
    assert p.stages == po.DEFAULT_STAGES == abi.POST_RECONSTRUCT | abi.POST_TEMPORAL | abi.POST_MOTION and list(p._reserved) == [0, 0, 0]
    d, r, t = abi.DenoiseConfig(), abi.ReconstructConfig(), abi.TemporalConfig()
    assert so.fovpt_denoise_defaults(C.byref(d)) == so.fovpt_reconstruct_defaults(C.byref(r)) == so.fovpt_temporal_defaults(C.byref(t)) == 0
    for mine, theirs in ((p.denoise, d), (p.reconstruct, r), (p.temporal, t)):
        assert bytes(mine) == bytes(theirs)
    assert so.fovpt_post_defaults(None) == -1


def test_post_rejects_null_arguments(so):
    p = abi.PostConfig()
    so.fovpt_post_defaults(C.byref(p))
    lp = abi.LaunchParams()
    assert so.fovpt_post(None, C.byref(lp), C.byref(p), None, None, None, None) == -1
    col, rgba = C.c_void_p(), C.c_void_p()
    assert so.fovpt_post_buffers(None, C.byref(col), C.byref(rgba)) == -1


# ---- the definition on two planes: a wall z = 10 facing a still pinhole camera, its right third a nearer plane z = 6 -----------
W, H, GAZE, RI, RO = 64, 48, (30, 22), 6, 16
CAM = dict(eye=(0.0, 0.0, 0.0), U=(1.0, 0.0, 0.0), V=(0.0, 0.75, 0.0), W=(0.0, 0.0, 1.0))


def _frame(seed, uniform=0):
    rng = np.random.default_rng(seed)
    d = tr.miss_dirs(W, H, CAM["U"], CAM["V"], CAM["W"])
    z = np.where(np.arange(W)[None, :] >= 2 * W // 3, f32(6.0), f32(10.0)).astype(np.float32)
    X = (d * z[..., None]).astype(np.float32)
    t = np.sqrt((X.astype(np.float64) ** 2).sum(-1)).astype(np.float32)
    nrm = np.zeros((H, W, 4), np.float32)
    nrm[..., 2] = -1.0
    alb = np.zeros((H, W, 4), np.float32)
    alb[..., :3] = rng.uniform(0.2, 0.9, (H, W, 3))
    gb = dict(prim=(np.arange(W)[None, :] >= 2 * W // 3).astype(np.uint32) * np.ones((H, 1), np.uint32),
              position=np.concatenate([X, t[..., None]], axis=-1).astype(np.float32), normal=nrm, albedo=alb)
    fill, pas, ax, ay = rr.writers(W, H, GAZE, RI, RO, uniform)
    inp = rng.uniform(0, 2, (H, W, 4)).astype(np.float32)          # (alpha is not 1: a carried pixel shows it)
    return dict(inp=inp, color=inp.copy(), normal=nrm, albedo=alb, gb=gb, uv=np.zeros((H, W, 2), np.float32), fill=fill, pas=pas,
                ax=ax, ay=ay, uniform=uniform, cam=CAM)


def _prev(frame, seed=4):
    hist = np.random.default_rng(seed).uniform(0, 2, (H, W, 4)).astype(np.float32)
    hist[..., 3] = 3.0
    return dict(gb=frame["gb"], cam=CAM, history=hist)


ONES = dict(history_fovea=1, history_middle=1, history_periphery=1, history_uniform=1)


def test_levels_0_and_caps_1_return_the_input_bit_for_bit():
    fr = _frame(1)
    assert {1, 2, 4} <= set(np.unique(fr["fill"]).tolist())
    for stages in (po.RECONSTRUCT | po.TEMPORAL, po.DEFAULT_STAGES):
        out = po.post(stages, fr, _prev(fr), dict(reconstruct=dict(levels=0), temporal=ONES))
        assert np.array_equal(bits(out["color"]), bits(fr["inp"]))
        assert np.array_equal(bits(out["history"][..., :3]), bits(fr["inp"][..., :3])) and (out["history"][..., 3] == 1).all()
        assert out["denoised"] is None and (out["motion"] is None) == (not stages & po.MOTION)
    # and with the caps open the same input is blended: the property above is not vacuous
    out = po.post(po.DEFAULT_STAGES, fr, _prev(fr), dict(reconstruct=dict(levels=0)))
    assert (out["history"][..., 3] > 1).mean() > 0.5 and not np.array_equal(bits(out["color"]), bits(fr["inp"]))


def test_an_unchanged_pixel_keeps_its_input_alpha_through_a_first_step():
    fr = _frame(2)
    for stages in (po.RECONSTRUCT | po.TEMPORAL, po.DEFAULT_STAGES):
        out = po.post(stages, fr, None, dict(reconstruct=dict(remodulate=0)))
        rec = rr.reconstruct(fr["inp"], fr["albedo"], fr["gb"], fr["fill"], fr["ax"], fr["ay"], dict(remodulate=0))
        kept = (bits(rec) == bits(fr["inp"])).all(axis=-1)
        assert kept[fr["fill"] <= 1].all() and kept.sum() >= 100 and (~kept).sum() >= 100      # (the fovea: ~ pi 7^2 pixels)
        assert np.array_equal(bits(out["color"][kept]), bits(fr["inp"][kept]))            # alpha included
        assert (out["color"][~kept][:, 3] == 1).all() and (fr["inp"][kept][:, 3] != 1).all()
        assert np.array_equal(bits(out["color"]), bits(rec)) and (out["history"][..., 3] == 1).all()
        if stages & po.MOTION:
            assert not out["motion"].any()


def test_the_stages_compose():
    """Each mask is the stage restatements one after the other; DENOISE feeds the later stages and ignores inp."""
    import denoise_ref as dn
    import temporal_motion_ref as tm
    fr, prev = _frame(3), None
    prev = _prev(fr)
    d = dict(dn.DEFAULTS)
    den, _ = dn.denoise(fr["color"], fr["normal"], fr["albedo"], fr["fill"], dn.iteration_map(fr["fill"], fr["pas"], d, 0), d)
    rec = rr.reconstruct(den, fr["albedo"], fr["gb"], fr["fill"], fr["ax"], fr["ay"])
    cap = tr.caps(fr["fill"], 0)
    want_c, want_h, want_m = tm.step(rec, fr["gb"], fr["uv"], cap, CAM, prev)
    other = dict(fr, inp=np.zeros_like(fr["inp"]))
    out = po.post(15, other, prev)
    assert np.array_equal(bits(out["denoised"]), bits(den)) and np.array_equal(bits(out["color"]), bits(want_c))
    assert np.array_equal(bits(out["history"]), bits(want_h)) and np.array_equal(bits(out["motion"]), bits(want_m))
    assert np.array_equal(bits(po.post(po.DENOISE, fr)["color"]), bits(den))
    assert np.array_equal(bits(po.post(po.DENOISE | po.RECONSTRUCT, fr)["color"]), bits(rec))
    plain = po.post(po.TEMPORAL, fr, prev)
    assert np.array_equal(bits(plain["color"]), bits(tr.step(fr["inp"], fr["gb"], cap, CAM, prev)[0])) and plain["motion"] is None
    for bad in (0, po.MOTION, po.MOTION | po.RECONSTRUCT, 16):
        with pytest.raises(ValueError):
            po.post(bad, fr)
