"""More GPU parity cases through the C ABI: committed goldens, the generic launch entry point with
the reference's edge behaviour (clamped off-frame writes, unsigned wrap, overlapping fills),
accumulate mode, shadow catchers, tile sharding, the C++ drop-in shim, error behaviour, and the
full-size benchmark configurations."""
import ctypes as C
import os

import numpy as np
import pytest

from fovpathtracing_optixcodelatest_amd import abi, lib, renderer, scenes

from common import cfg_foveated, cfg_uniform, compare_frames, make_gpu, make_oracle
from gpu_common import BOX_CAMERA, box_model, build_dropin, run_dropin

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_committed_golden_frames():
    g = np.load(os.path.join(GOLD, "frames.npz"))
    r = make_gpu(scenes.cornell_box(), scenes.ambient_probe(64, 32, 0.2), scenes.CORNELL_CAMERA, (64, 64), cfg_uniform(4, 3))
    r.render()
    assert _bits_equal(r.downloadAccum(), g["cornell_accum"]) and np.array_equal(r.downloadPixels(), g["cornell_frame"])
    r.close()
    r = make_gpu(scenes.cornell_box(), scenes.sky_probe(), scenes.CORNELL_CAMERA, (128, 72), cfg_foveated(10, 30, (1, 2, 8)))
    r.render()
    assert _bits_equal(r.downloadAccum(), g["fov_accum"]) and np.array_equal(r.downloadPixels(), g["fov_frame"])
    assert r.launchParams.frame.subframe_index == 1
    r.close()


def _launch_both(oracle, size, grid, setup, model=None, accumulate=0, prefill=None, max_depth=4):
    model = model or scenes.cornell_box()
    probe = scenes.sky_probe()
    cfg = abi.Config.reference_default()
    cfg.max_depth, cfg.accumulate = max_depth, accumulate
    r = make_gpu(model, probe, scenes.CORNELL_CAMERA, size, cfg)
    S, F = make_oracle(oracle, model, probe, scenes.CORNELL_CAMERA, size)
    for lp in (r.launchParams, F.lp):
        setup(lp)
    if prefill is not None:
        F.accum[...] = prefill
        # upload the same previous-frame accum to the device through a dummy uniform render is not
        # possible; use hipMemcpy via ctypes on the HIP runtime the library already loaded
        hip = C.CDLL("libamdhip64.so.7")            # by SONAME: the copy libfovpt.so is bound to, whichever that is
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(r.launchParams.frame.accum_buffer, prefill.ctypes.data, prefill.nbytes, 1) == 0
    r.launch(*grid)
    r.synchronize()
    oracle.launch(S, F, grid[0], grid[1], max_depth=max_depth, accumulate=accumulate)
    ga, gf = r.downloadAccum(), r.downloadPixels()
    r.close()
    return ga, gf, F.accum, F.frame


def test_launch_offframe_grid_is_clamped_like_the_reference(oracle):
    """Grid hanging over the right/bottom edge: writes are clamped onto the edge pixels
    (deviceProgram.cu:554); the last launch index in (y, x) order wins."""
    def setup(lp):
        f = lp.frame
        f.factor.x, f.factor.y, f.factor.z, f.fillSize = 2, 2, 1, 2
        f.r_inner, f.r_outer = 0.0, 1e9
        f.offset.x, f.offset.y, f.redraw = 40, 30, 0
        f.c.x, f.c.y = 48, 32
        lp.samples_per_launch = 2
    ga, gf, oa, of = _launch_both(oracle, (64, 48), (20, 16), setup)
    assert _bits_equal(ga, oa) and np.array_equal(gf, of)
    assert (ga[-1, 40:, 3] == 1).all() and (ga[30:, -1, 3] == 1).all() and (ga[:30, :40, 3] == 0).all()


def test_launch_unsigned_wrap_and_overlapping_fills(oracle):
    """Gaze near the corner: offset = c - r wraps in uint32 (SimplePathtracer.cpp:172); fill > factor
    makes neighbouring launch indices overwrite each other in launch order."""
    def setup(lp):
        f = lp.frame
        f.factor.x, f.factor.y, f.factor.z, f.fillSize = 2, 2, 1, 3
        f.r_inner, f.r_outer = 3.0, 14.0
        f.c.x, f.c.y = 5, 4
        f.offset.x, f.offset.y = (5 - 16) & 0xFFFFFFFF, (4 - 16) & 0xFFFFFFFF
        f.redraw = 1
        lp.samples_per_launch = 3
    ga, gf, oa, of = _launch_both(oracle, (48, 40), (16, 16), setup)
    assert _bits_equal(ga, oa) and np.array_equal(gf, of)
    assert (ga[..., 3] == 1).sum() > 50


def test_render_with_gaze_in_the_corner(oracle):
    cfg = cfg_foveated(10, 30, (1, 2, 4))
    size, gaze = (128, 96), (6, 90)
    r = make_gpu(scenes.cornell_box(), scenes.sky_probe(), scenes.CORNELL_CAMERA, size, cfg, gaze)
    r.render()
    S, F = make_oracle(oracle, scenes.cornell_box(), scenes.sky_probe(), scenes.CORNELL_CAMERA, size, gaze)
    oracle.render(S, F, cfg)
    assert _bits_equal(r.downloadAccum(), F.accum) and np.array_equal(r.downloadPixels(), F.frame)
    r.close()


def test_accumulate_mode_sv4_vmv2(oracle):
    """clamp(0,10) + running mean over subframes (PT_sv4_vmv2/deviceProgram.cu:545-553): only fires when
    subframe_index > 0 and redraw == 0."""
    rng = np.random.default_rng(3)
    prev = rng.uniform(0, 2, (48, 64, 4)).astype(np.float32)

    def setup(lp):
        f = lp.frame
        f.factor.x, f.factor.y, f.factor.z, f.fillSize = 4, 4, 1, 4
        f.r_inner, f.r_outer, f.redraw = 0.0, 1e9, 0
        f.subframe_index = 5
        lp.samples_per_launch = 2
    ga, gf, oa, of = _launch_both(oracle, (64, 48), (16, 12), setup, accumulate=1, prefill=prev)
    assert _bits_equal(ga, oa) and np.array_equal(gf, of)
    ga0, _, _, _ = _launch_both(oracle, (64, 48), (16, 12), setup, accumulate=0, prefill=prev)
    assert not _bits_equal(ga, ga0)


def test_shadow_catcher_material(oracle):
    """MATERIAL_FLAG_SHADOW_CATCHER: primary hits run SampleShadow into alpha, secondary hits pass
    through without consuming depth (deviceProgram.cu:646-651,691-694)."""
    m = scenes.cornell_box()
    m.meshes[0].material.flags = abi.MATERIAL_FLAG_SHADOW_CATCHER      # floor + ceiling + back wall
    size = (96, 96)
    cfg = cfg_uniform(4, 3)
    r = make_gpu(m, scenes.sky_probe(), scenes.CORNELL_CAMERA, size, cfg)
    r.render()
    S, F = make_oracle(oracle, m, scenes.sky_probe(), scenes.CORNELL_CAMERA, size)
    oracle.render(S, F, cfg)
    ga = r.downloadAccum()
    assert _bits_equal(ga, F.accum) and np.array_equal(r.downloadPixels(), F.frame)
    r.close()


def test_denoiser_guide_buffers(oracle):
    """write_guides: normal / color / albedo buffers as PT_sv/deviceProgram.cu:555-557 wrote them
    (first-hit normal and albedo averaged over the samples; commented out in PT_sv5_)."""
    model, probe, size = scenes.atrium(8000), scenes.ambient_probe(96, 54, 2.5), (192, 108)
    cfg = cfg_foveated(15, 48, (1, 2, 8))
    cfg.write_guides = 1
    r = make_gpu(model, probe, scenes.ATRIUM_CAMERA, size, cfg)
    r.render()
    f = r.launchParams.frame
    got = [r.download(ptr, np.empty((size[1], size[0], 4), np.float32)) for ptr in (f.normal_buffer, f.color_buffer, f.albedo_buffer)]
    ga = r.downloadAccum()
    r.close()
    S, F = make_oracle(oracle, model, probe, scenes.ATRIUM_CAMERA, size)
    oracle.render(S, F, cfg)
    assert _bits_equal(ga, F.accum)
    for g, o in zip(got, (F.normal, F.color, F.albedo)):
        assert _bits_equal(g, o)
    assert _bits_equal(got[1], ga)                                        # color_buffer == accum_buffer
    n = np.linalg.norm(got[0][..., :3], axis=-1)
    assert ((n > 0.99) & (n < 1.01)).mean() > 0.3                          # 1-spp periphery pixels carry unit normals


def test_two_rank_tile_shards_sum_to_the_full_frame():
    """fovpt_config.rank/world: the shards are disjoint, zero elsewhere, and add up bit-exactly."""
    model, probe, size = scenes.atrium(8000), scenes.ambient_probe(96, 54, 2.5), (192, 108)
    cfg = cfg_foveated(15, 48, (1, 2, 8))
    full = make_gpu(model, probe, scenes.ATRIUM_CAMERA, size, cfg)
    full.render()
    fa, ff = full.downloadAccum(), full.downloadPixels()
    full.close()
    for world in (2, 3):
        sa = np.zeros_like(fa)
        sf = np.zeros_like(ff).astype(np.uint64)
        cover = np.zeros(ff.shape, np.int32)
        for rank in range(world):
            c = cfg.copy()
            c.rank, c.world = rank, world
            r = make_gpu(model, probe, scenes.ATRIUM_CAMERA, size, c)
            r.render()
            a, f = r.downloadAccum(), r.downloadPixels()
            r.close()
            sa += a
            sf += f
            cover += (f != 0)
        assert (cover <= 1).all() and np.array_equal(cover == 1, ff != 0)     # disjoint; holes between rings stay holes
        assert _bits_equal(sa, fa) and np.array_equal(sf.astype(np.uint32), ff)


def test_cpp_dropin_shim_end_to_end(oracle, tmp_path):
    """The C++ SampleRenderer of include/SimplePathtracer.h, used as PT_sv5_/main.cpp uses the reference's."""
    exe, out = build_dropin(tmp_path, "shim_gpu_test"), str(tmp_path / "shim_out.bin")
    res = run_dropin(exe, out)
    assert "subframe_index=1" in res.stdout
    px = np.fromfile(out, np.uint32).reshape(96, 160)
    cam = BOX_CAMERA
    S, F = make_oracle(oracle, box_model(), scenes.ambient_probe(160, 96, 2.5), cam, (160, 96))
    oracle.render(S, F, cfg_foveated(12, 36, (1, 2, 8)))
    assert np.array_equal(px, F.frame)
    # the same program on an OBJ file: loadOBJ of include/Model.h (the library's host-side loader) -> SampleRenderer
    _write_textured_obj(tmp_path)
    run_dropin(exe, out, tmp_path / "s.obj")
    px = np.fromfile(out, np.uint32).reshape(96, 160)
    from fovpathtracing_optixcodelatest_amd import loaders
    S, F = make_oracle(oracle, loaders.load_obj(str(tmp_path / "s.obj")), scenes.ambient_probe(160, 96, 2.5), cam, (160, 96))
    oracle.render(S, F, cfg_foveated(12, 36, (1, 2, 8)))
    assert np.array_equal(px, F.frame)
    # ... and with the probe from a Radiance file: loadProbe's stbi_loadf replaced by fovpt_image_load_float4 (main.cpp:160-171)
    from common import encode_hdr_rle
    rng = np.random.default_rng(17)
    rgbe = rng.integers(1, 256, (16, 32, 4), dtype=np.uint8)
    rgbe[..., 3] = rng.integers(126, 131, (16, 32))
    (tmp_path / "sky.hdr").write_bytes(encode_hdr_rle(rgbe))
    run_dropin(exe, out, tmp_path / "s.obj", tmp_path / "sky.hdr")
    px = np.fromfile(out, np.uint32).reshape(96, 160)
    S, F = make_oracle(oracle, loaders.load_obj(str(tmp_path / "s.obj")), loaders.load_probe_texels(str(tmp_path / "sky.hdr")), cam, (160, 96))
    oracle.render(S, F, cfg_foveated(12, 36, (1, 2, 8)))
    assert np.array_equal(px, F.frame)


def test_cpp_host_gathers_over_rccl(tmp_path):
    """the multi-GPU transport reachable from the C++ host.  A C++ program drives SampleRenderer and the
    library's own RCCL gather (fovpt_comm_init / fovpt_gather_frame: pack -> ncclSend / ncclRecv on fovpt_stream() -> unpack)
    with a communicator of one rank, three frames back to back without host synchronisation: the gathered frame is the
    rendered frame."""
    exe, out = build_dropin(tmp_path, "rccl_gather_test", extra=["-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"]), str(tmp_path / "rccl_out.bin")
    res = run_dropin(exe, out)
    px = np.fromfile(out, np.uint32).reshape(2, 96, 160)
    assert (px[0] != 0).sum() > 0.9 * px[0].size
    assert np.array_equal(px[0], px[1]), res.stdout


def test_python_host_gathers_over_the_library_transport():
    """`bench.py --gather lib` in small: the library's own RCCL transport driven from python -- fovpt_comm_get_unique_id,
    fovpt_comm_init with a communicator of one rank, fovpt_gather_frame IN PLACE (the root gathers into the frame it rendered
    into) three frames back to back -- leaves the frame what the renderer alone produces."""
    size = (160, 96)
    cfg = cfg_foveated(12, 40, (1, 2, 4))
    model, probe = scenes.atrium(6000), scenes.ambient_probe(64, 32, 2.5)
    r = make_gpu(model, probe, scenes.ATRIUM_CAMERA, size, cfg)
    r.render()
    want = r.downloadPixels()
    r.comm_init(renderer.SampleRenderer.comm_unique_id(), 0, 1)
    fb = r.launchParams.frame.frame_buffer
    for _ in range(3):
        r.launchParams.frame.subframe_index = 0
        r.render_async()
        r.gather_frame(0, fb, fb)
    got = r.downloadPixels()
    r.comm_destroy()
    r.close()
    assert (want != 0).sum() > 0.9 * want.size and np.array_equal(got, want)


@pytest.mark.parametrize("budget", ["0.3", "1.0"])
def test_spatial_splits_do_not_change_the_frame(oracle, budget, monkeypatch):
    """Spatial splits in the hierarchy build (FOVPT_SPLIT: long triangles enter the build as several references, each a leaf
    record of the WHOLE triangle with its global primitive id -- replaces part of optixAccelBuild, SimplePathtracer.cpp:677-735):
    a ray may test a triangle more than once, and closest hit (minimum (t, primitive id)), the occlusion predicate, the frame
    and the ray counts stay what they are.  Scene: the hall plus four triangles that span it."""
    size = (160, 96)
    hall = scenes.atrium(6000)
    v = np.concatenate([m.vertex for m in hall.meshes])
    lo, hi = v.min(0), v.max(0)
    big = np.float32([[lo[0], lo[1] + 1.0, lo[2]], [hi[0], lo[1] + 1.0, lo[2]], [hi[0], lo[1] + 1.0, hi[2]], [lo[0], lo[1] + 1.0, hi[2]],
                      [lo[0], lo[1], lo[2]], [hi[0], hi[1], hi[2]], [lo[0], hi[1], hi[2]]])
    model = scenes.Model(list(hall.meshes) + [scenes.TriangleMesh(big, np.uint32([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 5]]), scenes.matte((0.6, 0.6, 0.5)))],
                         list(hall.textures))
    cfg = cfg_foveated(12, 40, (1, 2, 4))
    probe = scenes.sky_probe(64, 32, seed=9)
    r = make_gpu(model, probe, scenes.ATRIUM_CAMERA, size, cfg)
    r.render()
    want_a, want_f, st0 = r.downloadAccum(), r.downloadPixels(), r.stats()
    o, d = np.float32([[0, 100, 0]] * 3), np.float32([[0, -1, 0], [1, 0, 0], [0.577, 0.577, 0.577]])
    p0 = r.debug_trace(o, d)
    r.close()
    monkeypatch.setenv("FOVPT_SPLIT", budget)
    r = make_gpu(model, probe, scenes.ATRIUM_CAMERA, size, cfg)
    r.render()
    got_a, got_f, st1 = r.downloadAccum(), r.downloadPixels(), r.stats()
    p1 = r.debug_trace(o, d)
    r.close()
    assert st1.num_triangles == st0.num_triangles                       # the scene is the same; the build saw more references
    assert np.array_equal(got_a.view(np.uint32), want_a.view(np.uint32)) and np.array_equal(got_f, want_f)
    assert (st1.paths, st1.radiance_rays, st1.shadow_rays) == (st0.paths, st0.radiance_rays, st0.shadow_rays)
    assert np.array_equal(p0[0], p1[0]) and np.array_equal(p0[1].view(np.uint32), p1[1].view(np.uint32)) and np.array_equal(p0[2], p1[2])
    S, F = make_oracle(oracle, model, probe, scenes.ATRIUM_CAMERA, size)
    oracle.render(S, F, cfg)
    assert np.array_equal(got_f, F.frame)


def test_reinsertion_does_not_change_the_frame(oracle, monkeypatch):
    """Reinsertion rounds on the PLOC tree (bvh_build.hip k_reinsert_*: subtrees are taken out and put back where the tree's SAH cost
    falls most -- part of what replaces optixAccelBuild, SimplePathtracer.cpp:677-735) change the hierarchy and nothing else:
    closest hit (minimum (t, primitive id)), the occlusion predicate, the frame and the ray counts of a scene of facade modules
    and large foliage cards are the same without it (FOVPT_REINSERT=0), with the default rounds and with 40, and equal to the
    oracle's; the hierarchy itself is not the same (fewer or more wide nodes)."""
    size = (192, 108)
    model = scenes.street(24000, material="app")
    cfg = cfg_foveated(14, 46, (1, 2, 4))
    probe = scenes.sky_probe(64, 32, seed=5)
    rng = np.random.default_rng(77)
    v = np.concatenate([m.vertex for m in model.meshes])
    lo, hi = v.min(0), v.max(0)
    o = (lo + (hi - lo) * rng.random((4096, 3))).astype(np.float32)
    d = rng.normal(size=(4096, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    got = {}
    for rounds in ("0", None, "40"):
        if rounds is None:
            monkeypatch.delenv("FOVPT_REINSERT", raising=False)
        else:
            monkeypatch.setenv("FOVPT_REINSERT", rounds)
        r = make_gpu(model, probe, scenes.STREET_CAMERA, size, cfg)
        r.render()
        got[rounds] = (r.downloadAccum(), r.downloadPixels(), r.stats(), r.debug_trace(o, d))
        r.close()
    a0, f0, st0, p0 = got["0"]
    assert st0.radiance_rays > 0 and st0.shadow_rays > 0
    for rounds in (None, "40"):
        a1, f1, st1, p1 = got[rounds]
        assert np.array_equal(a1.view(np.uint32), a0.view(np.uint32)) and np.array_equal(f1, f0), rounds
        assert (st1.paths, st1.radiance_rays, st1.shadow_rays) == (st0.paths, st0.radiance_rays, st0.shadow_rays), rounds
        assert np.array_equal(p0[0], p1[0]) and np.array_equal(p0[1].view(np.uint32), p1[1].view(np.uint32)) and np.array_equal(p0[2], p1[2]), rounds
        assert st1.num_triangles == st0.num_triangles
    assert got[None][2].num_bvh_nodes != st0.num_bvh_nodes or got["40"][2].num_bvh_nodes != st0.num_bvh_nodes      # the tree did change
    S, F = make_oracle(oracle, model, probe, scenes.STREET_CAMERA, size)
    oracle.render(S, F, cfg)
    assert np.array_equal(f0, F.frame)


def _write_textured_obj(tmp_path):
    rng = np.random.default_rng(4)
    tex = rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)
    with open(tmp_path / "t.ppm", "wb") as f:
        f.write(b"P6\n8 8\n255\n" + tex.tobytes())
    (tmp_path / "s.mtl").write_text("newmtl floor\nKd 0.5 0.5 0.5\nmap_Kd t.ppm\nnewmtl box\nKd 0.9 0.3 0.1\nKe 2 2 2\n")
    obj = ["mtllib s.mtl", "v -5 0 -5", "v 5 0 -5", "v 5 0 5", "v -5 0 5", "vt 0 0", "vt 3 0", "vt 3 3", "vt 0 3",
           "usemtl floor", "f 1/1 4/4 3/3 2/2",
           "o box", "v -1 0 -1", "v 1 0 -1", "v 1 2 -1", "v -1 2 -1", "v -1 0 1", "v 1 0 1", "v 1 2 1", "v -1 2 1",
           "usemtl box", "f 5 8 7 6", "f 9 10 11 12", "f 5 9 12 8", "f 6 7 11 10", "f 8 12 11 7"]
    (tmp_path / "s.obj").write_text("\n".join(obj) + "\n")


def test_error_behaviour():
    r = renderer.SampleRenderer(scenes.cornell_box())
    r.render()                                     # size 0: silently returns (SimplePathtracer.cpp:81-82)
    r.resize((0, 0))                               # minimised window: no-op (:231)
    r.resize((32, 32))
    with pytest.raises(lib.FovptError) as e:       # no probe yet
        r.render()
    assert e.value.code == -4
    r.setProbe(renderer.ProbeData(scenes.sky_probe()).BuildCDF())
    r.setCamera(renderer.Camera(**{"eye": (278, 273, -800), "lookat": (278, 273, 0), "up": (0, 1, 0), "fovY": 40.0}))
    r.launchParams.samples_per_launch = 0
    r.launchParams.frame.fillSize = 1
    with pytest.raises(lib.FovptError):            # do{}while(--i) needs spp >= 1
        r.launch(8, 8)
    bad = abi.Config.reference_default()
    bad.max_depth = 0
    with pytest.raises(lib.FovptError):
        r.config = bad
    r.launchParams.traversable = 12345             # a handle this context never issued
    with pytest.raises(lib.FovptError) as e:
        r.render()
    assert e.value.code == -3
    r.close()


@pytest.mark.parametrize("name", ["C2", "C3"])
def test_full_size_benchmark_configs_against_oracle(oracle, name):
    """BASELINE.json configs[1] and configs[2] at full size: 1920x1080 on the ~262 k-triangle atrium.
    C2 = uniform 1 spp, diffuse-only materials; C3 = foveated 8/2/1, Material() defaults, full BSDF + NEE."""
    W, H = 1920, 1080
    if name == "C2":
        model, cfg = scenes.atrium(262144, material="diffuse"), cfg_uniform(1, 4)
    else:
        model, cfg = scenes.atrium(262144, material="app"), cfg_foveated(148, 482, (1, 2, 8))
    probe = scenes.ambient_probe(W, H, 2.5)
    r = make_gpu(model, probe, scenes.ATRIUM_CAMERA, (W, H), cfg)
    r.render()
    ga, gf = r.downloadAccum(), r.downloadPixels()
    st = r.stats()
    # idempotence: the shipped app renders every frame with subframe_index 0 (main.cpp:402-407)
    r.launchParams.frame.subframe_index = 0
    r.render()
    assert _bits_equal(r.downloadAccum(), ga)
    r.close()
    S, F = make_oracle(oracle, model, probe, scenes.ATRIUM_CAMERA, (W, H))
    cnt = oracle.render(S, F, cfg, nthreads=min(32, os.cpu_count() or 1))
    l2, bits, px = compare_frames(ga, gf, F.accum, F.frame)
    assert l2 <= 1e-4, l2
    assert bits == 0 and px == 0, (l2, bits, px)
    assert st.paths == cnt[2]
    assert st.radiance_rays <= cnt[0] and st.shadow_rays <= cnt[1]
    assert (st.radiance_rays, st.shadow_rays) == (cnt.lib_radiance, cnt.lib_shadow)      # exact ray accounting
    assert np.isfinite(ga).all()
    # the three rings do not tile the frame exactly: a 4x4 periphery block whose top-left corner is inside
    # r_outer is skipped although its far pixels lie beyond the middle ring (reference behaviour, kept)
    holes = (ga[..., 3] != 1).mean()
    assert holes == 0 if name == "C2" else holes < 0.01


@pytest.mark.parametrize("scene", ["atrium", "street"])
def test_bistro_class_scene_full_size_against_oracle(oracle, scene):
    """BASELINE.json configs[3] geometry on one GPU: ~3.8 M triangles (17-level wide BVH), 2560x1440,
    foveated 8/2/1 with radii 197/643.  Whole frame bit-exact against the oracle.  Two scenes: the hall re-tessellated,
    and the open street of facade modules and foliage cards (depth complexity, long rays) under an HDR sky."""
    W, H = 2560, 1440
    if scene == "atrium":
        model, probe, camera = scenes.atrium(3800000, material="app"), scenes.ambient_probe(W, H, 2.5), scenes.ATRIUM_CAMERA
    else:
        model, probe, camera = scenes.street(3800000, material="app"), scenes.sky_probe(512, 256, seed=5), scenes.STREET_CAMERA
    cfg = cfg_foveated(197, 643, (1, 2, 8))
    r = make_gpu(model, probe, camera, (W, H), cfg)
    r.render()
    ga, gf = r.downloadAccum(), r.downloadPixels()
    st = r.stats()
    r.close()
    assert st.num_triangles == model.num_triangles and st.bvh_max_depth <= 21
    S, F = make_oracle(oracle, model, probe, camera, (W, H))
    cnt = oracle.render(S, F, cfg, nthreads=min(32, os.cpu_count() or 1))
    l2, bits, px = compare_frames(ga, gf, F.accum, F.frame)
    assert l2 <= 1e-4 and bits == 0 and px == 0, (l2, bits, px)
    assert st.paths == cnt[2] == 1726659          # paths per frame of C4
    assert (st.radiance_rays, st.shadow_rays) == (cnt.lib_radiance, cnt.lib_shadow)


@pytest.mark.parametrize("name,size,radii,depth,world", [("C4", (2560, 1440), (197, 643), 4, 4), ("C5 (one eye)", (2160, 2160), (296, 964), 8, 8)])
def test_tile_split_of_the_multi_gpu_configurations_at_full_size(name, size, radii, depth, world):
    """BASELINE.json configs[3] and [4] as they are configured -- 4 / 8 GPUs, tile split, gather of the final framebuffer --
    with the ranks run one after the other on this one GPU: every rank renders only the launch indices it owns and packs the
    pixels it owns (fovpt_gather_pack); the root's unpack of the buffers is the unsharded frame bit for bit (which the
    full-size tests hold against the oracle), the ranks' ray counts add up to the single-GPU counts, and the shards are balanced."""
    import torch
    W, H = size
    model, probe, camera = scenes.atrium(3800000, material="app"), scenes.ambient_probe(W, H, 2.5), scenes.ATRIUM_CAMERA
    cfg = cfg_foveated(radii[0], radii[1], (1, 2, 8), max_depth=depth)
    r = make_gpu(model, probe, camera, (W, H), cfg)
    r.render()
    want = r.downloadPixels().copy()
    written = int((r.downloadAccum()[..., 3] == 1).sum())        # pixels some launch index writes (a few at the borders have none)
    st = r.stats()
    full = (st.paths, st.radiance_rays, st.shadow_rays)
    packed, rays, counts = [], [], None
    for rank in range(world):
        c = cfg.copy()
        c.rank, c.world = rank, world
        r.config = c
        r.reset_stats()
        counts = r.gather_plan()
        r.launchParams.frame.subframe_index = 0                    # the same frame again (render() advances it, main.cpp:402-407 resets it)
        r.render()
        s = r.stats()
        rays.append((s.paths, s.radiance_rays, s.shadow_rays))
        stride = (max(counts) + 63) // 64 * 64
        buf = torch.zeros(stride, dtype=torch.int32, device="cuda")
        r.gather_pack(r.launchParams.frame.frame_buffer, buf.data_ptr())
        r.synchronize()
        packed.append(buf)
    assert sum(counts) == written and max(counts) - min(counts) < 0.02 * max(counts)
    assert tuple(sum(x[k] for x in rays) for k in range(3)) == full
    assert max(x[1] + x[2] for x in rays) < 1.1 * (full[1] + full[2]) / world          # interleaved 8x4 tiles balance the rays
    c = cfg.copy()
    c.rank, c.world = 0, world
    r.config = c
    r.gather_plan()
    target = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    gathered = torch.stack(packed)
    r.gather_unpack(gathered.data_ptr(), gathered.shape[1], target.data_ptr())
    r.synchronize()
    assert np.array_equal(target.cpu().numpy().view(np.uint32).reshape(H, W), want)
    r.close()


@pytest.mark.parametrize("scene", ["atrium", "street"])
def test_c5_stereo_bistro_class_full_size_against_oracle(oracle, scene):
    """BASELINE.json configs[4] at full size on one GPU: ~3.8 M triangles, stereo 2 x 2160x2160 (two cameras
    +-32 mm apart with OpenXR-style off-centre frusta, two render() calls per frame as in
    OtherProjects_01/11HelloRaytracingOpenXR/main.cpp:892-955), per-eye foveation with radii 296/964, gaze at the
    eye's frame centre, depth 8.  Both eyes bit-exact against the oracle; 3,654,059 paths per eye."""
    W = H = 2160
    # the hall re-tessellated to 3.8 M triangles, both eyes; and the open street of facade modules and foliage cards under an
    # HDR sky -- ONE eye by default (the CPU oracle needs ~90 s per eye of it), both with FOVPT_TEST_C5_STREET=1
    if scene == "atrium":
        model, probe, cam = scenes.atrium(3800000, material="app"), scenes.ambient_probe(W, H, 2.5), scenes.ATRIUM_CAMERA
    else:
        model, probe, cam = scenes.street(3800000, material="app"), scenes.sky_probe(512, 256, seed=5), scenes.STREET_CAMERA
    cfg = cfg_foveated(296, 964, (1, 2, 8), max_depth=8)
    r = make_gpu(model, probe, cam, (W, H), cfg)
    S, F = make_oracle(oracle, model, probe, cam, (W, H))
    fwd = np.array(cam["lookat"], np.float64) - np.array(cam["eye"], np.float64)
    right = np.cross(fwd, np.array(cam["up"], np.float64))
    right /= np.linalg.norm(right)
    total_rays = 0
    eyes = ((-1.0, (-0.85, 0.70)), (1.0, (-0.70, 0.85)))                       # XrFovf angleLeft/Right, radians
    if scene == "street" and os.environ.get("FOVPT_TEST_C5_STREET") != "1":
        eyes = eyes[:1]
    for side, (al, ar) in eyes:
        eye = tuple(np.array(cam["eye"], np.float64) + side * 3.2 * right)        # +-32 mm in the scene's cm
        r.setCameraFov(eye, fwd, cam["up"], al, ar, 0.78, -0.78)
        F.lp.camera = r.launchParams.camera
        for lp in (r.launchParams, F.lp):
            lp.frame.subframe_index = 0
        r.reset_stats()
        r.render()
        ga, gf = r.downloadAccum(), r.downloadPixels()
        st = r.stats()
        cnt = oracle.render(S, F, cfg, nthreads=min(32, os.cpu_count() or 1))
        l2, bits, px = compare_frames(ga, gf, F.accum, F.frame)
        assert l2 <= 1e-4 and bits == 0 and px == 0, (side, l2, bits, px)
        assert st.paths == cnt[2] == 3654059, (st.paths, cnt[2])
        assert (st.radiance_rays, st.shadow_rays) == (cnt.lib_radiance, cnt.lib_shadow)
        assert np.isfinite(ga).all()
        total_rays += st.radiance_rays + st.shadow_rays
    assert total_rays > len(eyes) * 3654059
    r.close()


def test_c1_cornell_full_size_against_oracle(oracle):
    """BASELINE.json configs[0] at full size: Cornell box (32 triangles), 512x512, uniform 4 spp, depth 3."""
    model, probe = scenes.cornell_box(), scenes.ambient_probe(64, 32, 0.2)
    assert model.num_triangles == 32
    cfg = cfg_uniform(4, 3)
    r = make_gpu(model, probe, scenes.CORNELL_CAMERA, (512, 512), cfg)
    r.render()
    ga, gf, st = r.downloadAccum(), r.downloadPixels(), r.stats()
    r.close()
    S, F = make_oracle(oracle, model, probe, scenes.CORNELL_CAMERA, (512, 512))
    cnt = oracle.render(S, F, cfg, nthreads=min(32, os.cpu_count() or 1))
    l2, bits, px = compare_frames(ga, gf, F.accum, F.frame)
    assert l2 <= 1e-4 and bits == 0 and px == 0, (l2, bits, px)
    assert st.paths == cnt[2] == 512 * 512 * 4
    assert (st.radiance_rays, st.shadow_rays) == (cnt.lib_radiance, cnt.lib_shadow)


def test_obj_loaded_textured_scene(oracle, tmp_path):
    """OBJ + MTL + map_Kd through loaders.load_obj (loadOBJ semantics), rendered and checked: exercises the
    textured-albedo path (barycentric texcoords + bilinear fetch, deviceProgram.cu:655-670) on real loader output."""
    from fovpathtracing_optixcodelatest_amd import loaders
    _write_textured_obj(tmp_path)
    model = loaders.load_obj(str(tmp_path / "s.obj"))
    assert model.num_triangles == 12 and len(model.textures) == 1
    cam = dict(eye=(4.0, 3.0, 6.0), lookat=(0.0, 0.8, 0.0), up=(0.0, 1.0, 0.0), fovy=45.0)
    size, cfg = (160, 96), cfg_foveated(12, 36, (1, 2, 8))
    r = make_gpu(model, scenes.sky_probe(), cam, size, cfg)
    r.render()
    S, F = make_oracle(oracle, model, scenes.sky_probe(), cam, size)
    oracle.render(S, F, cfg)
    assert _bits_equal(r.downloadAccum(), F.accum) and np.array_equal(r.downloadPixels(), F.frame)
    r.close()


def test_probe_loaded_from_a_radiance_hdr_file(oracle, tmp_path):
    """loadProbe (main.cpp:160-171): texels decoded from an .hdr file feed ProbeSample / ProbeEval on both sides."""
    from common import encode_hdr_rle
    from fovpathtracing_optixcodelatest_amd import loaders
    rng = np.random.default_rng(7)
    rgbe = rng.integers(1, 256, (16, 32, 4), dtype=np.uint8)
    rgbe[..., 3] = rng.integers(126, 131, (16, 32))
    rgbe[3, 20:23] = (255, 250, 240, 137)                       # a small sun: high contrast for the CDF searches
    (tmp_path / "sky.hdr").write_bytes(encode_hdr_rle(rgbe))
    data = loaders.load_hdr(str(tmp_path / "sky.hdr"))
    size, cfg = (160, 96), cfg_foveated(12, 36, (1, 2, 8))
    r = make_gpu(scenes.cornell_box(), data, scenes.CORNELL_CAMERA, size, cfg)
    r.render()
    S, F = make_oracle(oracle, scenes.cornell_box(), data, scenes.CORNELL_CAMERA, size)
    oracle.render(S, F, cfg)
    assert _bits_equal(r.downloadAccum(), F.accum) and np.array_equal(r.downloadPixels(), F.frame)
    r.close()


def test_gltf_loaded_scene(oracle, tmp_path):
    """glTF -> Model through loaders.load_gltf (sutil::Scene's node rules), rendered on both sides."""
    import base64
    import json
    from fovpathtracing_optixcodelatest_amd import loaders
    quad = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], np.float32)
    idx = np.array([0, 2, 1, 0, 3, 2], np.uint16)
    blob = quad.tobytes() + idx.tobytes()
    uri = "data:application/octet-stream;base64," + base64.b64encode(blob).decode()
    g = {"asset": {"version": "2.0"}, "buffers": [{"byteLength": len(blob), "uri": uri}],
         "bufferViews": [{"buffer": 0, "byteOffset": 0, "byteLength": 48}, {"buffer": 0, "byteOffset": 48, "byteLength": 12}],
         "accessors": [{"bufferView": 0, "componentType": 5126, "count": 4, "type": "VEC3"},
                       {"bufferView": 1, "componentType": 5123, "count": 6, "type": "SCALAR"}],
         "materials": [{"pbrMetallicRoughness": {"baseColorFactor": [0.7, 0.7, 0.7, 1], "roughnessFactor": 0.6, "metallicFactor": 0.0}},
                       {"pbrMetallicRoughness": {"baseColorFactor": [0.9, 0.2, 0.1, 1], "roughnessFactor": 0.2, "metallicFactor": 0.8},
                        "emissiveFactor": [2, 2, 2]}],
         "meshes": [{"primitives": [{"attributes": {"POSITION": 0}, "indices": 1, "material": 0}]},
                    {"primitives": [{"attributes": {"POSITION": 0}, "indices": 1, "material": 1}]}],
         "nodes": [{"mesh": 0, "scale": [6, 1, 6]},
                   {"children": [2, 3], "translation": [0, 1.2, 0]},
                   {"mesh": 1, "rotation": [0.38268343, 0, 0, 0.92387953], "scale": [0.8, 1, 0.8]},
                   {"mesh": 1, "translation": [2.2, 0.4, -1], "rotation": [0, 0, 0.70710678, 0.70710678]}]}
    (tmp_path / "s.gltf").write_text(json.dumps(g))
    model = loaders.load_gltf(str(tmp_path / "s.gltf"))
    assert model.num_triangles == 6
    cam = dict(eye=(5.0, 4.0, 7.0), lookat=(0.0, 0.8, 0.0), up=(0.0, 1.0, 0.0), fovy=45.0)
    size, cfg = (160, 96), cfg_foveated(12, 36, (1, 2, 8))
    r = make_gpu(model, scenes.sky_probe(), cam, size, cfg)
    r.render()
    S, F = make_oracle(oracle, model, scenes.sky_probe(), cam, size)
    oracle.render(S, F, cfg)
    assert _bits_equal(r.downloadAccum(), F.accum) and np.array_equal(r.downloadPixels(), F.frame)
    assert int((r.downloadPixels() != 0).sum()) > 0.5 * size[0] * size[1]
    r.close()


def test_small_geometry_seen_from_far_away(oracle):
    """The box test of the traversal must stay conservative where its rounding errors are largest relative
    to the boxes: centimetre triangles around the origin and far off it, camera 1500 units away, narrow
    field of view.  A missed box would show up as a pixel that differs from the oracle."""
    rng = np.random.default_rng(11)
    n = 3000
    centre = np.concatenate([rng.uniform(-0.6, 0.6, (n // 2, 3)), rng.uniform(-0.6, 0.6, (n - n // 2, 3)) + np.float32([900.0, -700.0, 0.0])])
    tri = centre[:, None, :] + rng.uniform(-0.02, 0.02, (n, 3, 3))
    verts = tri.reshape(-1, 3).astype(np.float32)
    idx = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    model = scenes.Model(meshes=[scenes.TriangleMesh(vertex=verts, index=idx, material=scenes.matte((0.8, 0.7, 0.6), emission=(0.5, 0.5, 0.5)))])
    size, cfg = (192, 128), cfg_uniform(2, max_depth=3)
    for eye, lookat, fov in (((0.0, 0.0, 1500.0), (0.0, 0.0, 0.0), 0.055), ((900.0, -700.0, -1200.0), (900.0, -700.0, 0.0), 0.07)):
        cam = dict(eye=eye, lookat=lookat, up=(0.0, 1.0, 0.0), fovy=fov)
        r = make_gpu(model, scenes.ambient_probe(32, 16, 1.0), cam, size, cfg)
        r.render()
        S, F = make_oracle(oracle, model, scenes.ambient_probe(32, 16, 1.0), cam, size)
        oracle.render(S, F, cfg)
        assert _bits_equal(r.downloadAccum(), F.accum) and np.array_equal(r.downloadPixels(), F.frame)
        covered = int((F.accum[..., :3].sum(-1) > 1.0).sum())
        assert covered > 0.15 * size[0] * size[1]
        r.close()


@pytest.mark.gpu
def test_library_frames_against_the_python_path_tracer():
    """The product against tests/mini_pt.py directly, no oracle in between: the independent binary64 Python statement of the
    path (its own RNG, camera rays, brute-force hits, Disney BSDF, probe sampling, path loop, foveated launches) predicts the
    radiance the library renders -- uniform and three-pass foveated frames of the Cornell box with a shadow-catching floor."""
    import types
    import mini_pt
    model, cam = scenes.cornell_box(), scenes.CORNELL_CAMERA
    model.meshes[0].material.flags = abi.MATERIAL_FLAG_SHADOW_CATCHER      # floor + ceiling + back wall
    probe_data = scenes.sky_probe(16, 8, seed=6)
    for foveated in (False, True):
        w, h = (20, 20) if not foveated else (48, 32)
        cfg = cfg_uniform(2, max_depth=3) if not foveated else cfg_foveated(5, 11, (1, 2, 3), max_depth=3)
        gaze = (27, 14)
        r = make_gpu(model, probe_data, cam, (w, h), cfg, gaze=gaze, subframe_index=2)
        pd = renderer.ProbeData(probe_data).BuildCDF()
        hp = types.SimpleNamespace(data=pd.data, pdfx=pd.pdfValuesX, cdfx=pd.cdfValuesX, pdfy=pd.pdfValuesY, cdfy=pd.cdfValuesY)
        c = r.launchParams.camera
        uvw = [np.float64([v.x, v.y, v.z]) for v in (c.U, c.V, c.W)]
        r.render()
        got = r.downloadAccum().astype(np.float64)
        r.close()
        if foveated:
            want, doubtful = mini_pt.render_foveated(model, hp, uvw, cam["eye"], w, h, gaze, 5, 11, (1, 2, 3), 2, 3)
        else:
            want, doubtful = mini_pt.render_uniform(model, hp, uvw, cam["eye"], w, h, 2, 3)
        written = ~np.isnan(want[..., 0])
        assert np.array_equal(written, got[..., 3] == 1.0)
        err = np.abs(got[..., :3][written] - want[written]).max(1) / np.maximum(np.abs(want[written]).max(1), 0.05)
        assert (err < 1e-3).mean() > 0.97 and err[~doubtful[written]].max() < 1e-3 and np.median(err) < 1e-5, (foveated, float(np.median(err)))


@pytest.mark.gpu
def test_hierarchy_choice_does_not_change_the_frame(oracle, monkeypatch):
    """Hits are defined without reference to the hierarchy (closest t, lowest primitive id): the plain Karras
    LBVH (FOVPT_BVH=lbvh, the A/B path of fovpt_set_scene) must give the oracle's frame just as PLOC does."""
    model = scenes.atrium(20000)
    probe = scenes.sky_probe(64, 32, seed=3)
    size, cfg = (320, 180), cfg_foveated(24, 80, (1, 2, 8))
    S, F = make_oracle(oracle, model, probe, scenes.ATRIUM_CAMERA, size)
    oracle.render(S, F, cfg)
    nodes = {}
    for kind in ("ploc", "lbvh"):
        monkeypatch.setenv("FOVPT_BVH", kind)
        r = make_gpu(model, probe, scenes.ATRIUM_CAMERA, size, cfg)
        r.render()
        assert _bits_equal(r.downloadAccum(), F.accum) and np.array_equal(r.downloadPixels(), F.frame), kind
        nodes[kind] = r.stats().num_bvh_nodes
        r.close()
    assert 0 < nodes["ploc"] and 0 < nodes["lbvh"] and nodes["ploc"] != nodes["lbvh"]      # two different trees were built
    # ... nor does the order of a wide node's children (by default the one that ends occlusion rays soonest, k_order_children;
    # FOVPT_BVH_ORDER=0 keeps the order of the collapse), seen through the frame and ray by ray through the production kernel
    monkeypatch.setenv("FOVPT_BVH", "ploc")
    rng = np.random.default_rng(5)
    n = 4096
    org = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32) * np.float32([1700.0, 600.0, 800.0]) + np.float32([0.0, 700.0, 0.0])   # inside the atrium
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    traces = []
    for order in ("0", "1"):
        monkeypatch.setenv("FOVPT_BVH_ORDER", order)
        r = make_gpu(model, probe, scenes.ATRIUM_CAMERA, size, cfg)
        r.render()
        assert _bits_equal(r.downloadAccum(), F.accum) and np.array_equal(r.downloadPixels(), F.frame), order
        traces.append(r.debug_trace(org, d))
        r.close()
    for a, b in zip(traces[0], traces[1]):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
    assert 0.05 < np.mean(traces[0][2]) < 0.999                                            # (some of those rays are occluded, some not)


@pytest.mark.gpu
def test_degenerate_geometry_builds_a_shallow_hierarchy(oracle):
    """Tens of thousands of identical triangles (every box equal, every cost in the collapse tied) next to ordinary
    geometry: the build must not fail on depth, and the frame is still the oracle's (ties -> lowest primitive id)."""
    rng = np.random.default_rng(2)
    n_dup, n_rnd = 40000, 2000
    one = np.float32([[-0.5, -0.5, 0.0], [0.5, -0.5, 0.0], [0.0, 0.6, 0.0]])
    tri = np.concatenate([np.broadcast_to(one, (n_dup, 3, 3)),
                          rng.uniform(-2.0, 2.0, (n_rnd, 1, 3)) + rng.uniform(-0.2, 0.2, (n_rnd, 3, 3))]).astype(np.float32)
    verts = tri.reshape(-1, 3)
    idx = np.arange(verts.shape[0], dtype=np.uint32).reshape(-1, 3)
    model = scenes.Model(meshes=[scenes.TriangleMesh(vertex=verts, index=idx, material=scenes.matte((0.7, 0.6, 0.5), emission=(0.3, 0.3, 0.3)))])
    cam = dict(eye=(0.0, 0.0, 6.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fovy=40.0)
    size, cfg = (96, 64), cfg_uniform(1, max_depth=2)
    r = make_gpu(model, scenes.ambient_probe(32, 16, 1.0), cam, size, cfg)
    assert 0 < r.stats().bvh_max_depth <= 21
    # (the reinsertion search cannot prune among coincident boxes: its per-node visit budget keeps the build from going quadratic)
    assert r.stats().ms_bvh_build < 3000.0, r.stats().ms_bvh_build
    r.render()
    S, F = make_oracle(oracle, model, scenes.ambient_probe(32, 16, 1.0), cam, size)
    oracle.render(S, F, cfg)
    assert _bits_equal(r.downloadAccum(), F.accum) and np.array_equal(r.downloadPixels(), F.frame)
    r.close()


_FUZZ = range(int(os.environ.get("FOVPT_FUZZ_FROM", "0")), int(os.environ.get("FOVPT_FUZZ_TO", "40")))      # widen for a sweep


@pytest.mark.parametrize("seed", _FUZZ)
def test_random_configurations(oracle, seed):
    """Seeded random frame sizes (odd ones too), radii (zero, equal, larger than the frame), sample counts,
    depths, gaze points (also off the frame), subframe indices, uniform / foveated / accumulate, materials and
    probes: whatever the reference's code does with them, both sides must do the same."""
    rng = np.random.default_rng(1000 + seed)
    w, h = int(rng.integers(17, 150)), int(rng.integers(9, 100))
    model = scenes.cornell_box() if seed % 3 == 0 else scenes.atrium(int(rng.integers(300, 6000)), seed=int(rng.integers(1, 99)),
                                                                        material=("app", "diffuse", "matte")[seed % 3])
    cam = scenes.CORNELL_CAMERA if seed % 3 == 0 else scenes.ATRIUM_CAMERA
    probe = (scenes.sky_probe(), scenes.ambient_probe(w, h, 2.5), scenes.ambient_probe(16, 8, 0.7))[int(rng.integers(0, 3))]
    if rng.random() < 0.3:
        cfg = cfg_uniform(int(rng.integers(1, 6)), max_depth=int(rng.integers(1, 7)))
    else:
        r_i = int(rng.integers(0, 60))
        r_o = r_i + int(rng.integers(0, 120))                # (fovpt_set_config refuses r_outer < r_inner)
        cfg = cfg_foveated(r_i, r_o, tuple(int(x) for x in rng.integers(1, 7, 3)), max_depth=int(rng.integers(1, 7)))
    cfg.accumulate = int(rng.random() < 0.3)
    gaze = (int(rng.integers(-20, w + 20)), int(rng.integers(-20, h + 20)))
    sub = int(rng.integers(0, 4))
    r = make_gpu(model, probe, cam, (w, h), cfg, gaze=gaze, subframe_index=sub)
    S, F = make_oracle(oracle, model, probe, cam, (w, h), gaze=gaze, subframe_index=sub)
    want_rays = [0, 0, 0]
    for _ in range(2):                                   # two frames: subframe_index advances, accumulate blends
        r.render()
        cnt = oracle.render(S, F, cfg)
        want_rays = [want_rays[0] + cnt.lib_radiance, want_rays[1] + cnt.lib_shadow, want_rays[2] + cnt[2]]
        assert _bits_equal(r.downloadAccum(), F.accum) and np.array_equal(r.downloadPixels(), F.frame), (w, h, gaze, sub)
    st = r.stats()
    assert [st.radiance_rays, st.shadow_rays, st.paths] == want_rays          # exact ray accounting
    r.close()


_FUZZ_L = range(int(os.environ.get("FOVPT_FUZZL_FROM", "0")), int(os.environ.get("FOVPT_FUZZL_TO", "48")))


@pytest.mark.parametrize("seed", _FUZZ_L)
def test_random_single_launches(oracle, monkeypatch, seed):
    """fovpt_launch = one optixLaunch with caller-chosen parameters: random factor (also 3), fill (0 .. larger than
    the factor), offsets that wrap below zero or push the grid off the frame, rings, gaze points on and off the
    frame, grids smaller and larger than the frame, two launches into the same frame; every other seed with a
    job budget so small that the launch is cut into chunks of rows."""
    rng = np.random.default_rng(5000 + seed)
    if seed % 2:
        monkeypatch.setenv("FOVPT_SLOT_BUDGET", str(int(np.random.default_rng(seed).integers(400, 2500))))     # >= one launch row
    w, h = int(rng.integers(12, 90)), int(rng.integers(8, 70))
    model = scenes.cornell_box()
    probe = scenes.sky_probe()
    cfg = abi.Config.reference_default()
    cfg.max_depth, cfg.accumulate = int(rng.integers(1, 4)), int(rng.random() < 0.3)
    r = make_gpu(model, probe, scenes.CORNELL_CAMERA, (w, h), cfg)
    S, F = make_oracle(oracle, model, probe, scenes.CORNELL_CAMERA, (w, h))
    for launch_no in range(2):
        fx, fy = (int(v) for v in rng.integers(1, 5, 2))
        fill = int(rng.integers(0, 6))
        gaze = (int(rng.integers(-8, w + 8)) & 0xFFFFFFFF, int(rng.integers(-8, h + 8)) & 0xFFFFFFFF)
        off = (int(rng.integers(-30, w)) & 0xFFFFFFFF, int(rng.integers(-30, h)) & 0xFFFFFFFF)
        r_i = float(rng.integers(0, 20))
        r_o = 1e9 if rng.random() < 0.4 else r_i + float(rng.integers(0, 60))
        gw, gh = int(rng.integers(1, w // fx + 12)), int(rng.integers(1, h // fy + 12))
        spp, sub, redraw = int(rng.integers(1, 4)), int(rng.integers(0, 3)), int(rng.integers(0, 2))
        for lp in (r.launchParams, F.lp):
            f = lp.frame
            f.factor.x, f.factor.y, f.factor.z, f.fillSize = fx, fy, 1, fill
            f.r_inner, f.r_outer = r_i, r_o
            f.c.x, f.c.y = gaze
            f.offset.x, f.offset.y = off
            f.redraw, f.subframe_index = redraw, sub
            lp.samples_per_launch = spp
        r.launch(gw, gh)
        r.synchronize()
        oracle.launch(S, F, gw, gh, max_depth=cfg.max_depth, accumulate=cfg.accumulate)
        assert _bits_equal(r.downloadAccum(), F.accum) and np.array_equal(r.downloadPixels(), F.frame), \
            (seed, launch_no, (w, h), (fx, fy), fill, gaze, off, (r_i, r_o), (gw, gh), spp, sub, redraw)
    r.close()


_FUZZ_M = range(int(os.environ.get("FOVPT_FUZZM_FROM", "0")), int(os.environ.get("FOVPT_FUZZM_TO", "32")))


@pytest.mark.parametrize("seed", _FUZZ_M)
def test_random_shards_chunks_and_guides(oracle, monkeypatch, seed):
    """Random frame configurations run (a) as world = 2..8 tile shards with random tile sizes, (b) cut into chunks
    by a small job budget, (c) with the denoiser guide buffers on: shards add up to the oracle's frame, chunked
    and unchunked frames are the oracle's frame, guides are the oracle's guides."""
    rng = np.random.default_rng(9000 + seed)
    w, h = int(rng.integers(40, 160)), int(rng.integers(24, 100))
    model = scenes.atrium(int(rng.integers(500, 6000)), seed=int(rng.integers(1, 99)))
    probe = scenes.sky_probe() if seed % 2 else scenes.ambient_probe(w, h, 2.5)
    if rng.random() < 0.25:
        cfg = cfg_uniform(int(rng.integers(1, 4)), max_depth=int(rng.integers(1, 5)))
    else:
        r_i = int(rng.integers(2, 30))
        cfg = cfg_foveated(r_i, r_i + int(rng.integers(1, 60)), tuple(int(x) for x in rng.integers(1, 6, 3)), max_depth=int(rng.integers(1, 5)))
    gaze = (int(rng.integers(0, w)), int(rng.integers(0, h)))
    S, F = make_oracle(oracle, model, probe, scenes.ATRIUM_CAMERA, (w, h), gaze=gaze)
    gcfg = cfg.copy(); gcfg.write_guides = 1
    oracle.render(S, F, gcfg)
    # (c) guides + the plain frame
    r = make_gpu(model, probe, scenes.ATRIUM_CAMERA, (w, h), gcfg, gaze=gaze)
    r.render()
    f = r.launchParams.frame
    for ptr, want in ((f.normal_buffer, F.normal), (f.color_buffer, F.color), (f.albedo_buffer, F.albedo)):
        assert _bits_equal(r.download(ptr, np.empty((h, w, 4), np.float32)), want)
    assert _bits_equal(r.downloadAccum(), F.accum) and np.array_equal(r.downloadPixels(), F.frame)
    r.close()
    # (a) shards
    world = int(rng.integers(2, 9))
    tile = (int(rng.integers(1, 17)), int(rng.integers(1, 9)))
    total_f = np.zeros((h, w), np.uint64); total_a = np.zeros((h, w, 4), np.float32)
    for rank in range(world):
        c = cfg.copy()
        c.rank, c.world, c.tile_w, c.tile_h = rank, world, tile[0], tile[1]
        rr = make_gpu(model, probe, scenes.ATRIUM_CAMERA, (w, h), c, gaze=gaze)
        rr.render()
        total_f += rr.downloadPixels(); total_a += rr.downloadAccum()
        rr.close()
    assert np.array_equal(total_f.astype(np.uint32), F.frame) and _bits_equal(total_a, F.accum), (world, tile)
    # (b) chunks
    monkeypatch.setenv("FOVPT_SLOT_BUDGET", str(int(rng.integers(600, 5000))))
    rc = make_gpu(model, probe, scenes.ATRIUM_CAMERA, (w, h), cfg, gaze=gaze)
    rc.render()
    assert _bits_equal(rc.downloadAccum(), F.accum) and np.array_equal(rc.downloadPixels(), F.frame)
    rc.close()


_FUZZ_S = range(int(os.environ.get("FOVPT_FUZZS_FROM", "0")), int(os.environ.get("FOVPT_FUZZS_TO", "40")))


@pytest.mark.parametrize("seed", _FUZZ_S)
def test_random_scenes_and_materials(oracle, seed):
    """Random triangle soups with duplicated and coplanar-overlapping triangles (closest-hit ties: lowest primitive
    id), zero-area triangles, several meshes with random Disney parameters over their whole ranges (transmission 0
    and 1, eta 0, subsurface, clearcoat, roughness 0 ...), emitters, textured meshes, sometimes a shadow catcher."""
    rng = np.random.default_rng(7000 + seed)
    meshes = []
    textures = []
    nmesh = int(rng.integers(1, 6))
    for m in range(nmesh):
        n = int(rng.integers(1, 200))
        centre = rng.uniform(-4, 4, (n, 1, 3)) * np.float32([1.0, 0.4, 1.0])
        tri = centre + rng.uniform(-1.2, 1.2, (n, 3, 3))
        if n > 4:
            tri[1] = tri[0]                                       # exact duplicate: the lower primitive id wins
            tri[2] = tri[0] + np.float32([0.3, 0.0, 0.1]) * 0.0 + (tri[0][1] - tri[0][0]) * 0.25   # coplanar, shifted along an edge
            tri[3][2] = tri[3][1]                                 # zero area
        v = tri.reshape(-1, 3).astype(np.float32)
        idx = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
        mat = abi.Material.reference_default()
        mat.color.set(rng.uniform(0, 1, 3)); mat.emission.set(rng.uniform(0, 3, 3) if rng.random() < 0.3 else (0, 0, 0))
        pick = lambda *vals: float(vals[int(rng.integers(0, len(vals)))])
        mat.transmission = pick(0.0, 1.0, rng.uniform(0, 1)); mat.metallic = pick(0.0, 1.0, rng.uniform(0, 1))
        mat.roughness = pick(0.0, 1.0, rng.uniform(0, 1)); mat.subsurface = pick(0.0, 0.0, rng.uniform(0, 1))
        mat.specular = pick(0.0, 1.0, rng.uniform(0, 1)); mat.specularTint = pick(0.0, 1.0, rng.uniform(0, 1))
        mat.clearcoat = pick(0.0, 1.0, rng.uniform(0, 1)); mat.clearcoatGloss = pick(0.0, 1.0, rng.uniform(0, 1))
        mat.eta = pick(0.0, 1.0, 1.5, rng.uniform(1, 2))
        if m == 0 and rng.random() < 0.3:
            mat.flags = abi.MATERIAL_FLAG_SHADOW_CATCHER
        tc, tid = None, -1
        if rng.random() < 0.5:
            tw, th = int(rng.integers(1, 9)), int(rng.integers(1, 9))           # any size, not only powers of two
            textures.append(rng.integers(0, 2 ** 32, (th, tw), dtype=np.uint64).astype(np.uint32))
            tid = len(textures) - 1
            tc = rng.uniform(-2, 3, (3 * n, 2)).astype(np.float32)             # wraps in both directions
        meshes.append(scenes.TriangleMesh(vertex=v, index=idx, material=mat, texcoord=tc, texture_id=tid))
    model = scenes.Model(meshes=meshes, textures=textures)
    cam = dict(eye=(0.0, 2.5, 11.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fovy=50.0)
    size = (int(rng.integers(40, 120)), int(rng.integers(30, 90)))
    cfg = cfg_uniform(int(rng.integers(1, 4)), max_depth=int(rng.integers(1, 6)))
    probe = scenes.sky_probe() if seed % 2 else scenes.ambient_probe(32, 16, 1.0)
    if seed % 5 == 4:
        # a hostile environment map: black rows and columns (zero row sums: BuildCDF divides 0 by 0 exactly as
        # the reference does), a few very bright texels
        probe = rng.uniform(0, 1, (12, 24, 4)).astype(np.float32) ** 4
        probe[..., 3] = 1.0
        probe[int(rng.integers(0, 12))] = (0, 0, 0, 1)
        probe[:, int(rng.integers(0, 24))] = (0, 0, 0, 1)
        probe[int(rng.integers(0, 12)), int(rng.integers(0, 24)), :3] = 5000.0
    r = make_gpu(model, probe, cam, size, cfg)
    r.render()
    S, F = make_oracle(oracle, model, probe, cam, size)
    cnt = oracle.render(S, F, cfg)
    assert _bits_equal(r.downloadAccum(), F.accum) and np.array_equal(r.downloadPixels(), F.frame)
    assert r.stats().paths == cnt[2]
    r.close()
