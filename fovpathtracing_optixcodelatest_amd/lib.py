"""Loader for libfovpt.so (the HIP C-ABI library, include/fovpt.h).

There is no CPU fallback: if the library is missing or a call fails, an exception is raised.
"""
import ctypes as C
import os
import subprocess

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO_PATH = os.environ.get("FOVPT_SO") or os.path.join(CSRC, "libfovpt.so")   # FOVPT_SO: A/B builds of the same library

EXPORTS = [
    "fovpt_create", "fovpt_destroy", "fovpt_last_error", "fovpt_set_scene", "fovpt_set_probe", "fovpt_set_probe_data",
    "fovpt_resize", "fovpt_get_config", "fovpt_set_config", "fovpt_launch", "fovpt_render",
    "fovpt_synchronize", "fovpt_download", "fovpt_get_stats", "fovpt_reset_stats", "fovpt_stream",
    "fovpt_probe_build_cdf", "fovpt_camera_uvw", "fovpt_debug_math", "fovpt_debug_buffer", "fovpt_debug_trace",
    "fovpt_debug_probe_sample", "fovpt_debug_probe_eval", "fovpt_debug_bsdf", "fovpt_debug_tex2d", "fovpt_debug_resolve", "fovpt_debug_shade",
    "fovpt_debug_generate", "fovpt_debug_build", "fovpt_debug_trace_queued",
    "fovpt_gather_plan", "fovpt_gather_pack", "fovpt_gather_unpack",
    "fovpt_denoise_defaults", "fovpt_denoise", "fovpt_denoise_buffers",
    "fovpt_gbuffer", "fovpt_reconstruct_defaults", "fovpt_reconstruct", "fovpt_reconstruct_buffers",
    "fovpt_temporal_defaults", "fovpt_temporal", "fovpt_temporal_motion", "fovpt_temporal_buffers", "fovpt_temporal_reset", "fovpt_update_vertices",
    "fovpt_update_transforms", "fovpt_hierarchy_cost", "fovpt_rebuild_state", "fovpt_set_skins", "fovpt_update_skinned",
    "fovpt_set_morphs", "fovpt_update_morphed", "fovpt_set_rig", "fovpt_update_animated",
    "fovpt_post_defaults", "fovpt_post", "fovpt_post_buffers",
    "fovpt_expose_defaults", "fovpt_expose", "fovpt_expose_buffers", "fovpt_expose_state", "fovpt_expose_reset",
    "fovpt_bloom_defaults", "fovpt_bloom", "fovpt_bloom_buffers",
    "fovpt_warp_defaults", "fovpt_warp", "fovpt_warp_buffers", "fovpt_warp_counts", "fovpt_temporal_gbuffer",
    "fovpt_warp_motion_defaults", "fovpt_warp_motion",
    "fovpt_focus_defaults", "fovpt_focus", "fovpt_focus_buffers", "fovpt_focus_state", "fovpt_focus_reset",
    "fovpt_lens_defaults", "fovpt_lens", "fovpt_lens_buffers",
    "fovpt_variance_defaults", "fovpt_variance", "fovpt_variance_buffers", "fovpt_variance_reset",
    "fovpt_variance_filter_defaults", "fovpt_variance_filter", "fovpt_variance_filter_buffers",
    "fovpt_quality_defaults", "fovpt_quality", "fovpt_quality_read", "fovpt_quality_host",
    "fovpt_quality_mse", "fovpt_quality_psnr", "fovpt_quality_ssim", "fovpt_quality_score",
    "fovpt_packet_describe", "fovpt_packet_encode", "fovpt_packet_submit", "fovpt_packet_wait", "fovpt_packet_decode",
    "fovpt_packet_check", "fovpt_packet_decode_host",
    "fovpt_packet_defaults", "fovpt_packet_describe_coded", "fovpt_packet_encode_coded", "fovpt_packet_submit_coded",
    "fovpt_comm_get_unique_id", "fovpt_comm_init", "fovpt_comm_destroy", "fovpt_gather_frame",
    "fovpt_model_load_obj", "fovpt_model_load_gltf", "fovpt_model_destroy", "fovpt_model_counts", "fovpt_model_get_mesh", "fovpt_model_get_texture",
    "fovpt_image_load_float4", "fovpt_image_free", "fovpt_image_load_rgba8", "fovpt_image_free_rgba8",
]


class FovptError(RuntimeError):
    """The std::runtime_error of the reference (sutil::Exception, sutil/Exception.h:245)."""

    def __init__(self, code, msg):
        super().__init__("libfovpt error %d: %s" % (code, msg))
        self.code = code


def build(force=False):
    """Compile libfovpt.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC, "-s", "-j4"]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return SO_PATH


_lib = None


def _share_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's, found by file name
    through an RPATH).  Imported FIRST, torch's copy also serves libfovpt.so; imported AFTER libfovpt.so has
    pulled in /opt/rocm's copy, torch loads a second HIP/HSA runtime into the process, which finds "No HIP
    GPUs".  So when torch is installed but not imported yet, its copy is loaded here, and either import order
    ends with one runtime.  Without torch (C++ callers, plain Python) the library binds to /opt/rocm as linked.
    FOVPT_SYSTEM_HIP=1 skips this."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("FOVPT_SYSTEM_HIP"):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    hip = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(hip):
        try:
            C.CDLL(hip, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def share_torch_rccl():
    """The same for RCCL, before the library's own transport (fovpt_comm_*) loads one: PyTorch bundles a librccl.so of its own
    (another file than /opt/rocm's librccl.so.1) and the library takes whichever copy the process already holds: with torch
    installed but not imported yet, torch's copy is loaded here, so that either order ends with one RCCL.  Loaded RTLD_LOCAL, as
    the library loads it: RCCL brings librocm_smi64 along, whose `amd::smi` globals also exist in /opt/rocm's libamd_smi.so
    (which torch's device queries load) -- made global, the two run their static destructors on one object and the process
    aborts with a double free when it exits (round 4: this transport first, `import torch` afterwards).
    FOVPT_SYSTEM_HIP=1 or FOVPT_RCCL_LIB skip this."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("FOVPT_SYSTEM_HIP") or os.environ.get("FOVPT_RCCL_LIB"):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    rccl = os.path.join(list(spec.submodule_search_locations)[0], "lib", "librccl.so")
    if os.path.exists(rccl):
        try:
            C.CDLL(rccl)
        except OSError:
            pass


def _declare_loader(L):
    """The signatures both libraries share: fovpt_last_error and the scene / image ingestion (fovpt_model_*, fovpt_image_*)."""
    vp, i32 = C.c_void_p, C.c_int
    L.fovpt_last_error.argtypes = [vp]
    L.fovpt_last_error.restype = C.c_char_p
    L.fovpt_model_load_obj.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.fovpt_model_load_gltf.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.fovpt_model_destroy.argtypes = [vp]
    L.fovpt_model_destroy.restype = None
    L.fovpt_model_counts.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.fovpt_model_get_mesh.argtypes = [vp, i32, C.POINTER(abi.ModelMesh)]
    L.fovpt_model_get_texture.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(i32), C.POINTER(i32)]
    L.fovpt_image_load_float4.argtypes = [C.c_char_p, C.POINTER(i32), C.POINTER(i32), C.POINTER(vp)]
    L.fovpt_image_free.argtypes = [vp]
    L.fovpt_image_free.restype = None
    L.fovpt_image_load_rgba8.argtypes = [C.c_char_p, C.POINTER(i32), C.POINTER(i32), C.POINTER(vp)]
    L.fovpt_image_free_rgba8.argtypes = [vp]
    L.fovpt_image_free_rgba8.restype = None


def _declare_packet_host(L):
    """The packet entry points both libraries share: the checks and the decoder for a client (csrc/packet_host.cpp)."""
    L.fovpt_packet_check.argtypes = [C.c_void_p, C.c_size_t]
    L.fovpt_packet_decode_host.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_int, C.c_int]
    for name in PACKET_HOST_EXPORTS:
        getattr(L, name).restype = C.c_int


def _declare_quality_host(L):
    """The quality entry points both libraries share: the measurement on host images and the scores of a record
    (csrc/quality_host.cpp)."""
    sums = C.POINTER(abi.QualitySums)
    L.fovpt_quality_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(abi.QualityConfig), sums]
    L.fovpt_quality_host.restype = C.c_int
    for name in QUALITY_SCORE_EXPORTS:
        getattr(L, name).argtypes = [sums, C.POINTER(C.c_double) if name == "fovpt_quality_score" else C.c_int]
        getattr(L, name).restype = C.c_double


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise FovptError(-100, "%s is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)" % SO_PATH)
    _share_torch_hip_runtime()
    L = C.CDLL(SO_PATH)
    vp, i32, u32, u64, sz = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_size_t
    L.fovpt_create.argtypes = [C.POINTER(vp), i32]
    L.fovpt_destroy.argtypes = [vp]
    L.fovpt_destroy.restype = None
    L.fovpt_set_scene.argtypes = [vp, vp, i32, vp, i32, C.POINTER(u64)]
    L.fovpt_set_probe.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(abi.Probe)]
    L.fovpt_set_probe_data.argtypes = [vp, i32, i32, vp, vp, C.POINTER(abi.Probe)]
    L.fovpt_resize.argtypes = [vp, i32, i32, C.POINTER(abi.FramePtrs)]
    L.fovpt_get_config.argtypes = [vp, C.POINTER(abi.Config)]
    L.fovpt_set_config.argtypes = [vp, C.POINTER(abi.Config)]
    L.fovpt_launch.argtypes = [vp, C.POINTER(abi.LaunchParams), u32, u32]
    L.fovpt_render.argtypes = [vp, C.POINTER(abi.LaunchParams)]
    L.fovpt_synchronize.argtypes = [vp]
    L.fovpt_download.argtypes = [vp, vp, vp, sz]
    L.fovpt_get_stats.argtypes = [vp, C.POINTER(abi.Stats)]
    L.fovpt_reset_stats.argtypes = [vp]
    L.fovpt_stream.argtypes = [vp]
    L.fovpt_stream.restype = vp
    L.fovpt_probe_build_cdf.argtypes = [i32, i32, vp, vp, vp, vp, vp]
    L.fovpt_camera_uvw.argtypes = [C.POINTER(abi.Float3), C.POINTER(abi.Float3), C.POINTER(abi.Float3),
                                   C.c_float, C.c_float, C.POINTER(abi.Float3), C.POINTER(abi.Float3), C.POINTER(abi.Float3)]
    L.fovpt_gather_plan.argtypes = [vp, C.POINTER(abi.LaunchParams), vp, i32]
    L.fovpt_gather_pack.argtypes = [vp, vp, vp]
    L.fovpt_gather_unpack.argtypes = [vp, vp, u32, vp]
    L.fovpt_denoise_defaults.argtypes = [C.POINTER(abi.DenoiseConfig)]
    L.fovpt_denoise.argtypes = [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.DenoiseConfig), vp, vp]
    L.fovpt_denoise_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.fovpt_gbuffer.argtypes = [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.GBufferPtrs)]
    L.fovpt_reconstruct_defaults.argtypes = [C.POINTER(abi.ReconstructConfig)]
    L.fovpt_reconstruct.argtypes = [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.ReconstructConfig), vp, vp, vp]
    L.fovpt_reconstruct_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.fovpt_temporal_defaults.argtypes = [C.POINTER(abi.TemporalConfig)]
    L.fovpt_temporal.argtypes = [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.TemporalConfig), vp, vp, vp]
    L.fovpt_temporal_motion.argtypes = [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.TemporalConfig), vp, vp, vp, vp]
    L.fovpt_temporal_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.fovpt_temporal_reset.argtypes = [vp]
    L.fovpt_post_defaults.argtypes = [C.POINTER(abi.PostConfig)]
    L.fovpt_post.argtypes = [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.PostConfig), vp, vp, vp, vp]
    L.fovpt_post_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.fovpt_expose_defaults.argtypes = [C.POINTER(abi.ExposeConfig)]
    L.fovpt_expose.argtypes = [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.ExposeConfig), vp, vp, vp]
    L.fovpt_expose_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.fovpt_expose_state.argtypes = [vp, C.POINTER(abi.ExposeState)]
    L.fovpt_expose_reset.argtypes = [vp]
    L.fovpt_bloom_defaults.argtypes = [C.POINTER(abi.BloomConfig)]
    L.fovpt_bloom.argtypes = [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.BloomConfig), vp, vp, vp]
    L.fovpt_bloom_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.fovpt_warp_defaults.argtypes = [C.POINTER(abi.WarpConfig)]
    L.fovpt_warp.argtypes = [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.WarpCamera), C.POINTER(abi.WarpConfig), C.POINTER(abi.GBufferPtrs),
                             vp, vp, vp, vp, vp]
    L.fovpt_warp_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.fovpt_warp_counts.argtypes = [vp, C.POINTER(abi.WarpCounts)]
    L.fovpt_temporal_gbuffer.argtypes = [vp, C.POINTER(abi.GBufferPtrs)]
    L.fovpt_warp_motion_defaults.argtypes = [C.POINTER(abi.WarpMotionConfig)]
    L.fovpt_warp_motion.argtypes = [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.WarpCamera), C.POINTER(abi.WarpMotionConfig),
                                    C.POINTER(abi.GBufferPtrs), vp, vp, vp, vp, vp]
    L.fovpt_focus_defaults.argtypes = [C.POINTER(abi.FocusConfig)]
    L.fovpt_focus.argtypes = [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.FocusConfig), C.POINTER(abi.GBufferPtrs), vp, vp, vp, vp]
    L.fovpt_focus_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.fovpt_focus_state.argtypes = [vp, C.POINTER(abi.FocusState)]
    L.fovpt_focus_reset.argtypes = [vp]
    L.fovpt_lens_defaults.argtypes = [C.POINTER(abi.LensConfig)]
    L.fovpt_lens.argtypes = [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.LensConfig), C.POINTER(abi.WarpCamera), vp, vp, vp]
    L.fovpt_lens_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.fovpt_variance_defaults.argtypes = [C.POINTER(abi.VarianceConfig)]
    L.fovpt_variance.argtypes = [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.VarianceConfig), C.POINTER(abi.GBufferPtrs), vp, vp, vp]
    L.fovpt_variance_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.fovpt_variance_reset.argtypes = [vp]
    L.fovpt_variance_filter_defaults.argtypes = [C.POINTER(abi.VarianceFilterConfig)]
    L.fovpt_variance_filter.argtypes = [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.VarianceFilterConfig), C.POINTER(abi.GBufferPtrs), vp, vp, vp, vp]
    L.fovpt_variance_filter_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.fovpt_quality_defaults.argtypes = [C.POINTER(abi.QualityConfig)]
    L.fovpt_quality.argtypes = [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.QualityConfig), vp, vp, vp, vp]
    L.fovpt_quality_read.argtypes = [vp, C.POINTER(abi.QualitySums)]
    L.fovpt_packet_describe.argtypes =[vp, C.POINTER(abi.LaunchParams), u32, C.POINTER(abi.PacketHeader)]
    L.fovpt_packet_encode.argtypes = [vp, C.POINTER(abi.LaunchParams), vp, u32, vp]
    L.fovpt_packet_submit.argtypes = [vp, C.POINTER(abi.LaunchParams), vp, u32, C.POINTER(i32)]
    L.fovpt_packet_wait.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz)]
    L.fovpt_packet_decode.argtypes = [vp, C.POINTER(abi.PacketHeader), vp, i32, vp]
    L.fovpt_packet_defaults.argtypes = [C.POINTER(abi.PacketConfig)]
    L.fovpt_packet_defaults.restype = None
    L.fovpt_packet_describe_coded.argtypes = [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.PacketConfig), u32, C.POINTER(abi.PacketHeader)]
    L.fovpt_packet_encode_coded.argtypes = [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.PacketConfig), vp, u32, vp]
    L.fovpt_packet_submit_coded.argtypes = [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.PacketConfig), vp, u32, C.POINTER(i32)]
    L.fovpt_update_vertices.argtypes = [vp, C.POINTER(abi.VertexUpdate), i32, i32]
    L.fovpt_update_transforms.argtypes = [vp, C.POINTER(abi.MeshTransform), i32, i32]
    L.fovpt_hierarchy_cost.argtypes = [vp, i32, C.POINTER(abi.HierarchyCost)]
    L.fovpt_rebuild_state.argtypes = [vp, i32, C.POINTER(abi.RebuildInfo)]
    L.fovpt_set_skins.argtypes = [vp, C.POINTER(abi.MeshSkin), i32]
    L.fovpt_update_skinned.argtypes = [vp, C.POINTER(abi.SkinPose), i32, i32]
    L.fovpt_set_morphs.argtypes = [vp, C.POINTER(abi.MeshMorph), i32]
    L.fovpt_update_morphed.argtypes = [vp, C.POINTER(abi.MorphPose), i32, i32]
    L.fovpt_set_rig.argtypes = [vp, C.POINTER(abi.RigDesc)]
    L.fovpt_update_animated.argtypes = [vp, i32, C.c_float, i32]
    L.fovpt_comm_get_unique_id.argtypes = [vp]
    L.fovpt_comm_init.argtypes = [vp, vp, i32, i32]
    L.fovpt_comm_destroy.argtypes = [vp]
    L.fovpt_gather_frame.argtypes = [vp, C.POINTER(abi.LaunchParams), i32, vp, vp]
    L.fovpt_debug_math.argtypes = [vp, i32, vp, vp, vp, sz]
    L.fovpt_debug_buffer.argtypes = [vp, C.c_char_p, C.POINTER(vp), C.POINTER(sz)]
    L.fovpt_debug_trace.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.fovpt_debug_trace_queued.argtypes = [vp, C.POINTER(abi.DebugTraceLaunch), C.POINTER(abi.DebugTraceResult)]
    L.fovpt_debug_probe_sample.argtypes = [vp, C.POINTER(abi.Probe), i32, i32, vp, vp, vp, C.POINTER(i32)]
    L.fovpt_debug_probe_eval.argtypes = [vp, C.POINTER(abi.Probe), i32, i32, vp, vp, C.POINTER(i32)]
    L.fovpt_debug_bsdf.argtypes = [vp, C.POINTER(abi.Material), i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.fovpt_debug_tex2d.argtypes = [vp, i32, i32, vp, vp]
    L.fovpt_debug_shade.argtypes = [vp, C.POINTER(abi.Probe), C.POINTER(abi.DebugShadeLaunch), vp, vp, vp, vp, vp, vp, C.POINTER(abi.DebugShadeResult)]
    L.fovpt_debug_resolve.argtypes = [vp, C.POINTER(abi.LaunchParams), i32, u32, u32, C.POINTER(abi.DebugPass), C.POINTER(i32), vp, vp, vp, vp, vp, vp,
                                      C.POINTER(u32)]
    L.fovpt_debug_generate.argtypes = [vp, C.POINTER(abi.LaunchParams), C.POINTER(abi.DebugGenerateLaunch), C.POINTER(abi.DebugPass), C.POINTER(i32),
                                       C.POINTER(abi.DebugGenerateResult)]
    L.fovpt_debug_build.argtypes = [vp, u32, vp, vp, C.POINTER(abi.DebugBuildSwitches), C.POINTER(abi.DebugBuildTrace)]
    _declare_loader(L)
    _declare_packet_host(L)
    for name in EXPORTS:
        if name not in ("fovpt_destroy", "fovpt_last_error", "fovpt_stream", "fovpt_model_destroy", "fovpt_image_free", "fovpt_image_free_rgba8") + QUALITY_SCORE_EXPORTS:
            getattr(L, name).restype = i32
    _declare_quality_host(L)
    _lib = L
    return L


LOADER_SO_PATH = os.path.join(CSRC, "libfovpt_loader.so")
LOADER_EXPORTS = [n for n in EXPORTS if n.startswith("fovpt_model_") or n.startswith("fovpt_image_")] + ["fovpt_last_error"]
PACKET_HOST_EXPORTS = ["fovpt_packet_check", "fovpt_packet_decode_host"]      # in both libraries too
QUALITY_SCORE_EXPORTS = ("fovpt_quality_mse", "fovpt_quality_psnr", "fovpt_quality_ssim", "fovpt_quality_score")   # return a double
QUALITY_HOST_EXPORTS = ["fovpt_quality_host"] + list(QUALITY_SCORE_EXPORTS)   # in both libraries too
_loader = None


def load_loader():
    """The scene / image ingestion of the C ABI (fovpt_model_*, fovpt_image_*), the packet decoder for a client
    (PACKET_HOST_EXPORTS) and the quality measurement on host images (QUALITY_HOST_EXPORTS).  If libfovpt.so is already loaded, it; otherwise the
    HOST-ONLY libfovpt_loader.so (same code, g++, no HIP runtime), so that reading OBJ / glTF / JPEG / HDR files needs no GPU
    stack; FOVPT_SO (an A/B build of the whole library) takes precedence.  The render path never goes through here."""
    global _loader
    if _lib is not None or os.environ.get("FOVPT_SO") or not os.path.exists(LOADER_SO_PATH):
        return load()
    if _loader is not None:
        return _loader
    L = C.CDLL(LOADER_SO_PATH)
    _declare_loader(L)
    _declare_packet_host(L)
    _declare_quality_host(L)
    for name in LOADER_EXPORTS:
        if name not in ("fovpt_last_error", "fovpt_model_destroy", "fovpt_image_free", "fovpt_image_free_rgba8"):
            getattr(L, name).restype = C.c_int
    _loader = L
    return L


def check(ctx, rc, L=None):
    """Raises FovptError with the library's text; `L`: the library the failing call was made in (the loader library keeps its own
    error text)."""
    if rc != 0:
        msg = (L or load()).fovpt_last_error(ctx)
        raise FovptError(rc, msg.decode("utf-8", "replace") if msg else "")
