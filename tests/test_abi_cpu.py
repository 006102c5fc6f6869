"""CPU tests of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/fovpt.h declares, layouts match, the C++ shim compiles, and the product fails loudly
(no CPU fallback) when there is no GPU."""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest

import header_layout
from fovpathtracing_optixcodelatest_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def so():
    lib.build()
    return lib.load()


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "fovpt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fovpt_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(so):
    names = _declared_functions()
    assert len(names) >= 18
    for n in names:
        assert hasattr(so, n), "include/fovpt.h declares %s but libfovpt.so does not export it" % n
    assert sorted(lib.EXPORTS) == names


def test_host_only_loader_library(so, tmp_path):
    """csrc/libfovpt_loader.so: the scene / image ingestion of the C ABI as a host-only shared object -- it exports
    every fovpt_model_* / fovpt_image_* entry point of include/fovpt.h, depends on no HIP / HSA library, and a fresh interpreter
    that only reads files through the python loaders never maps libfovpt.so or the HIP runtime."""
    path = lib.LOADER_SO_PATH
    assert os.path.exists(path), "make -C csrc builds libfovpt_loader.so beside libfovpt.so"
    L = C.CDLL(path)
    wanted = [n for n in _declared_functions() if n.startswith("fovpt_model_") or n.startswith("fovpt_image_")]
    assert len(wanted) >= 10 and sorted(wanted + ["fovpt_last_error"]) == sorted(lib.LOADER_EXPORTS)
    for n in wanted:
        assert hasattr(L, n), n
    deps = subprocess.run(["ldd", path], capture_output=True, text=True).stdout
    assert "hip" not in deps.lower() and "hsa" not in deps.lower() and "rocm" not in deps.lower(), deps
    (tmp_path / "t.ppm").write_bytes(b"P6\n2 1\n255\n" + bytes([255, 0, 0, 0, 0, 255]))
    (tmp_path / "m.mtl").write_text("newmtl m\nKd 1 1 1\nmap_Kd t.ppm\n")
    (tmp_path / "m.obj").write_text("mtllib m.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nusemtl m\nf 1/1 2/1 3/1\n")
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from fovpathtracing_optixcodelatest_amd import loaders\n"
            "m = loaders.load_obj_native(%r)\n"
            "assert len(m.meshes) == 1 and len(m.textures) == 1 and m.textures[0].shape == (1, 2)\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert 'libfovpt_loader.so' in maps and 'libfovpt.so' not in maps and 'libamdhip64' not in maps, maps[-2000:]\n"
            % (ROOT, str(tmp_path / "m.obj")))
    env = {k: v for k, v in os.environ.items() if k != "FOVPT_SO"}
    res = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stderr[-2000:]


def test_struct_layouts_match_reference_abi():
    assert C.sizeof(abi.Material) == 104          # Material.h:48-69
    assert C.sizeof(abi.Probe) == 64              # Probe.cuh:6-21
    assert C.sizeof(abi.LaunchParams) == 248      # LaunchParams.h:49-91 with nvcc alignments
    assert abi.LaunchParams.camera.offset == 104
    assert abi.LaunchParams.samples_per_launch.offset == 152
    assert abi.LaunchParams.traversable.offset == 160
    assert abi.LaunchParams.probe.offset == 168
    assert abi.LaunchParams.white.offset == 240
    assert abi.Material.transmission.offset == 80 and abi.Material.flags.offset == 100
    m = abi.Material.reference_default()          # Material.h:13-38 constructor defaults
    assert (m.transmission, m.metallic, m.eta, m.roughness) == pytest.approx((0.4, 0.5, 1.4, 1.0))
    assert m.emission.tolist() == [1.0, 1.0, 1.0] and m.color.tolist() == [1.0, 0.0, 0.0]


def test_cpp_headers_compile_and_assert_layouts():
    for src in ("shim_compile_check.cpp",):
        header_layout.syntax_check_file(os.path.join(ROOT, "tests", "cpp", src))
    # the plain-C view of the header must compile as C too
    header_layout.syntax_check('#include "fovpt.h"\nint main(void){return sizeof(fovpt_launch_params)==248?0:1;}\n', lang="c99")


CPP_PROGRAMS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "tests", "cpp", "*.cpp")))
assert len(CPP_PROGRAMS) >= 33, "tests/cpp/*.cpp not found"        # (here, not in a case: no programs would mean no cases to fail)


@pytest.mark.parametrize("name", CPP_PROGRAMS)
def test_every_cpp_program_of_the_tests_compiles(name):
    """Each tests/cpp/*.cpp passes the compiler's syntax pass against include/ and the library's sources, so a slip in a program
    or in tests/cpp/box_scene.h shows where there is no GPU to run it on."""
    header_layout.syntax_check_file(os.path.join(ROOT, "tests", "cpp", name),
                               include=[os.path.join(ROOT, "fovpathtracing_optixcodelatest_amd", "csrc")])


def test_config_mirror_matches_the_header():
    """abi.Config is fovpt_config member for member (the header compiled by gcc says where each member lies)."""
    names = [f[0] for f in abi.Config._fields_]
    got = header_layout.layout("fovpt_config", abi.Config)
    assert got[0] == C.sizeof(abi.Config)
    assert got[1:] == [getattr(abi.Config, n).offset for n in names]


def test_debug_hook_structs_mirror_the_header():
    """The structs of the test hooks (fovpt_debug_pass, fovpt_debug_shade_*, fovpt_debug_generate_*, fovpt_debug_trace_*) member for
    member."""
    pairs = (("fovpt_debug_pass", abi.DebugPass), ("fovpt_debug_shade_launch", abi.DebugShadeLaunch), ("fovpt_debug_shade_result", abi.DebugShadeResult),
             ("fovpt_debug_generate_launch", abi.DebugGenerateLaunch), ("fovpt_debug_generate_result", abi.DebugGenerateResult),
             ("fovpt_debug_build_switches", abi.DebugBuildSwitches), ("fovpt_debug_build_trace", abi.DebugBuildTrace),
             ("fovpt_debug_trace_launch", abi.DebugTraceLaunch), ("fovpt_debug_trace_result", abi.DebugTraceResult))
    lines = header_layout.layouts(*pairs)
    assert len(lines) == len(pairs)
    for got, (cname, mirror) in zip(lines, pairs):
        assert got[0] == C.sizeof(mirror), cname
        assert got[1:] == [getattr(mirror, f[0]).offset for f in mirror._fields_], cname
    assert C.sizeof(abi.DebugGenerateLaunch) == 36 and C.sizeof(abi.DebugGenerateResult) == 120 and abi.DebugGenerateResult.count.offset == 56
    assert C.sizeof(abi.DebugTraceLaunch) == 296 and abi.DebugTraceLaunch.n.offset == 96 and abi.DebugTraceLaunch.decoy.offset == 260
    assert C.sizeof(abi.DebugTraceResult) == 80 and abi.DebugTraceResult.stat_radiance.offset == 40


def test_debug_trace_constants_mirror_the_header():
    """FOVPT_DEBUG_TRACE_ALPHA and FOVPT_DEBUG_TRACE_ITERS as the header compiled by gcc has them."""
    assert header_layout.constants("FOVPT_DEBUG_TRACE_ALPHA", "FOVPT_DEBUG_TRACE_ITERS") == [abi.DEBUG_TRACE_ALPHA, abi.DEBUG_TRACE_ITERS]


def test_default_config_is_the_shipped_reference(so):
    c = abi.Config.reference_default()
    assert (c.uniform, c.r_inner, c.r_outer) == (0, 74, 241)                 # SimplePathtracer.cpp:20-23
    assert (c.spp_periphery, c.spp_middle, c.spp_fovea, c.spp_uniform) == (8, 16, 32, 4)   # :142,170,193,95
    assert c.max_depth == 4                                                     # deviceProgram.cu:515


def test_host_helpers_reject_bad_arguments(so):
    assert so.fovpt_probe_build_cdf(0, 4, None, None, None, None, None) != 0
    assert so.fovpt_camera_uvw(None, None, None, 45.0, 1.0, None, None, None) != 0
    assert so.fovpt_set_config(None, None) != 0
    assert so.fovpt_render(None, None) != 0


def test_fails_loudly_without_gpu(so):
    """No CPU fallback: without a HIP device the constructor raises (initOptix, SimplePathtracer.cpp:320-321)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from fovpathtracing_optixcodelatest_amd import renderer, scenes
    with pytest.raises(lib.FovptError) as e:
        renderer.SampleRenderer(scenes.cornell_box())
    assert "no HIP device" in str(e.value)


def test_product_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "fovpathtracing_optixcodelatest_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert "oracle_py" not in text and "libfovpt_oracle" not in text and "orc_" not in text, f
    for f in os.listdir(os.path.join(ROOT, "include")):
        p = os.path.join(ROOT, "include", f)
        if os.path.isfile(p):
            assert "orc_" not in open(p).read()


def test_a_failing_dlopen_of_rccl_is_an_error_not_a_crash(so):
    """ADVICE r4, first item: rccl() asked dlerror() twice and gave the second answer, NULL, to a std::string, so the first
    candidate that failed to load ended the process.  A fresh process whose FOVPT_RCCL_LIB names no file must come back from
    fovpt_comm_get_unique_id: with another candidate's RCCL (FOVPT_OK), or with an error code and a reason."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import ctypes\n"
            "from fovpathtracing_optixcodelatest_amd import lib\n"
            "L = lib.load()\n"
            "buf = ctypes.create_string_buffer(256)\n"
            "rc = L.fovpt_comm_get_unique_id(buf)\n"
            "msg = L.fovpt_last_error(None) or b''\n"
            "print('RESULT', rc, len(msg), flush=True)\n" % ROOT)
    env = dict(os.environ, FOVPT_RCCL_LIB="/nonexistent/librccl.so")
    res = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT")]
    assert line, res.stdout[-2000:]
    rc, nmsg = (int(x) for x in line[-1].split()[1:])
    assert rc == 0 or nmsg > 0, "error code %d without a message" % rc


# every ctypes mirror of abi.py and the C type of include/fovpt.h it restates ("struct x": a type the header does not typedef,
# because a function has its name)
MIRRORS = {
    abi.Float3: "fovpt_float3", abi.Float4: "fovpt_float4", abi.Int2: "fovpt_int2", abi.UInt2: "fovpt_uint2", abi.UInt3: "fovpt_uint3",
    abi.Material: "fovpt_material", abi.Probe: "fovpt_probe", abi.LaunchParams: "fovpt_launch_params", abi.MeshDesc: "fovpt_mesh_desc",
    abi.TextureDesc: "fovpt_texture_desc", abi.ModelMesh: "fovpt_model_mesh", abi.Config: "fovpt_config", abi.Stats: "fovpt_stats",
    abi.FramePtrs: "fovpt_frame_ptrs", abi.VertexUpdate: "fovpt_vertex_update", abi.MeshTransform: "fovpt_mesh_transform",
    abi.HierarchyCost: "fovpt_hierarchy_cost_info", abi.RebuildInfo: "fovpt_rebuild_info", abi.MeshSkin: "fovpt_mesh_skin",
    abi.SkinPose: "fovpt_skin_pose", abi.MorphTarget: "fovpt_morph_target", abi.MeshMorph: "fovpt_mesh_morph", abi.MorphPose: "fovpt_morph_pose",
    abi.RigNode: "fovpt_rig_node", abi.RigBinding: "fovpt_rig_binding", abi.RigChannel: "fovpt_rig_channel", abi.RigClip: "fovpt_rig_clip",
    abi.RigDesc: "fovpt_rig_desc", abi.DenoiseConfig: "fovpt_denoise_config", abi.ReconstructConfig: "fovpt_reconstruct_config",
    abi.GBufferPtrs: "fovpt_gbuffer_ptrs", abi.TemporalConfig: "fovpt_temporal_config", abi.PostConfig: "fovpt_post_config",
    abi.ExposeConfig: "fovpt_expose_config", abi.ExposeState: "struct fovpt_expose_state", abi.BloomConfig: "fovpt_bloom_config",
    abi.WarpCamera: "fovpt_warp_camera", abi.WarpConfig: "fovpt_warp_config", abi.WarpMotionConfig: "fovpt_warp_motion_config",
    abi.WarpCounts: "struct fovpt_warp_counts", abi.FocusConfig: "fovpt_focus_config", abi.FocusState: "struct fovpt_focus_state",
    abi.LensConfig: "fovpt_lens_config", abi.VarianceConfig: "fovpt_variance_config", abi.VarianceFilterConfig: "fovpt_variance_filter_config",
    abi.QualityConfig: "fovpt_quality_config", abi.QualitySums: "fovpt_quality_sums", abi.PacketPass: "fovpt_packet_pass",
    abi.PacketConfig: "fovpt_packet_config", abi.PacketHeader: "fovpt_packet_header", abi.DebugPass: "fovpt_debug_pass",
    abi.DebugShadeLaunch: "fovpt_debug_shade_launch", abi.DebugShadeResult: "fovpt_debug_shade_result",
    abi.DebugTraceLaunch: "fovpt_debug_trace_launch", abi.DebugTraceResult: "fovpt_debug_trace_result",
    abi.DebugGenerateLaunch: "fovpt_debug_generate_launch", abi.DebugGenerateResult: "fovpt_debug_generate_result",
    abi.DebugBuildSwitches: "fovpt_debug_build_switches", abi.DebugBuildTrace: "fovpt_debug_build_trace",
}
RENAMED = {abi.PacketHeader: {"passes": "pass"}}          # (a mirror field whose C member has another name)
# the two members of fovpt_launch_params that are structs without a name of their own: pinned as members of it
NESTED = {abi._Frame: "frame", abi._Camera: "camera"}
NO_C_COUNTERPART = [abi.Struct]                             # the base class of the mirrors: copy() and as_dict(), no fields


def test_every_mirror_is_pinned_to_the_header():
    """sizeof and every field offset of every ctypes.Structure subclass defined in abi.py against the header compiled by gcc, and
    no such class outside the tables above: a struct added to abi.py is pinned here or this fails."""
    defined = [c for c in vars(abi).values() if isinstance(c, type) and issubclass(c, C.Structure) and c.__module__ == abi.__name__]
    assert len(defined) == len(set(defined)) >= 60
    assert sorted(c.__name__ for c in defined) == sorted(c.__name__ for c in list(MIRRORS) + list(NESTED) + NO_C_COUNTERPART)
    mirrors = list(MIRRORS)
    got = header_layout.layouts(*[(MIRRORS[m], m, RENAMED.get(m, {})) for m in mirrors])
    for m, lay in zip(mirrors, got):
        assert lay == header_layout.offsets(m), (m.__name__, MIRRORS[m])
    for m, member in NESTED.items():
        names = [f[0] for f in m._fields_]
        (lay,), (size,) = header_layout.probe([("fovpt_launch_params", ["%s.%s" % (member, n) for n in names])],
                                              ["sizeof(((fovpt_launch_params*)0)->%s)" % member])
        base = getattr(abi.LaunchParams, member).offset
        assert size == C.sizeof(m) and lay[1:] == [base + getattr(m, n).offset for n in names], m.__name__
    for c in NO_C_COUNTERPART:
        assert not hasattr(c, "_fields_")
