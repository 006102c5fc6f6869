"""Loader for libfovpt.so (the HIP C-ABI library, include/fovpt.h).

There is no CPU fallback: if the library is missing or a call fails, an exception is raised.
"""
import ctypes as C
import os
import subprocess

from . import abi, abi_depth

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO_PATH = os.environ.get("FOVPT_SO") or os.path.join(CSRC, "libfovpt.so")   # FOVPT_SO: A/B builds of the same library

_vp, _i32, _u32, _u64, _sz, _f32, _f64, _str, _P = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_size_t, C.c_float, C.c_double, C.c_char_p, C.POINTER
_params, _gbuf, _cam, _sums = _P(abi.LaunchParams), _P(abi.GBufferPtrs), _P(abi.WarpCamera), _P(abi.QualitySums)
_own2 = [_vp, _P(_vp), _P(_vp)]                # fovpt_<stage>_buffers: the context and two out-pointers


# Every entry point of include/fovpt.h: name -> (restype, argtypes).  The one statement of the C signatures on the Python side.
SIGNATURES = {
    # -- context, scene, frame loop
    "fovpt_create": (_i32, [_P(_vp), _i32]),
    "fovpt_destroy": (None, [_vp]),
    "fovpt_last_error": (_str, [_vp]),
    "fovpt_set_scene": (_i32, [_vp, _vp, _i32, _vp, _i32, _P(_u64)]),
    "fovpt_set_probe": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _P(abi.Probe)]),
    "fovpt_set_probe_data": (_i32, [_vp, _i32, _i32, _vp, _vp, _P(abi.Probe)]),
    "fovpt_resize": (_i32, [_vp, _i32, _i32, _P(abi.FramePtrs)]),
    "fovpt_get_config": (_i32, [_vp, _P(abi.Config)]),
    "fovpt_set_config": (_i32, [_vp, _P(abi.Config)]),
    "fovpt_launch": (_i32, [_vp, _params, _u32, _u32]),
    "fovpt_render": (_i32, [_vp, _params]),
    "fovpt_synchronize": (_i32, [_vp]),
    "fovpt_download": (_i32, [_vp, _vp, _vp, _sz]),
    "fovpt_get_stats": (_i32, [_vp, _P(abi.Stats)]),
    "fovpt_reset_stats": (_i32, [_vp]),
    "fovpt_stream": (_vp, [_vp]),
    "fovpt_probe_build_cdf": (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "fovpt_camera_uvw": (_i32, [_P(abi.Float3), _P(abi.Float3), _P(abi.Float3), _f32, _f32, _P(abi.Float3), _P(abi.Float3), _P(abi.Float3)]),
    # -- multi-GPU gather and its RCCL transport
    "fovpt_gather_plan": (_i32, [_vp, _params, _vp, _i32]),
    "fovpt_gather_pack": (_i32, [_vp, _vp, _vp]),
    "fovpt_gather_unpack": (_i32, [_vp, _vp, _u32, _vp]),
    "fovpt_comm_get_unique_id": (_i32, [_vp]),
    "fovpt_comm_init": (_i32, [_vp, _vp, _i32, _i32]),
    "fovpt_comm_destroy": (_i32, [_vp]),
    "fovpt_gather_frame": (_i32, [_vp, _params, _i32, _vp, _vp]),
    # -- post-frame stages (csrc/api_post.hip)
    "fovpt_denoise_defaults": (_i32, [_P(abi.DenoiseConfig)]),
    "fovpt_denoise": (_i32, [_vp, _params, _P(abi.DenoiseConfig), _vp, _vp]),
    "fovpt_denoise_buffers": (_i32, _own2),
    "fovpt_gbuffer": (_i32, [_vp, _params, _gbuf]),
    "fovpt_reconstruct_defaults": (_i32, [_P(abi.ReconstructConfig)]),
    "fovpt_reconstruct": (_i32, [_vp, _params, _P(abi.ReconstructConfig), _vp, _vp, _vp]),
    "fovpt_reconstruct_buffers": (_i32, _own2),
    "fovpt_temporal_defaults": (_i32, [_P(abi.TemporalConfig)]),
    "fovpt_temporal": (_i32, [_vp, _params, _P(abi.TemporalConfig), _vp, _vp, _vp]),
    "fovpt_temporal_buffers": (_i32, [_vp, _P(_vp), _P(_vp), _P(_vp)]),
    "fovpt_temporal_motion": (_i32, [_vp, _params, _P(abi.TemporalConfig), _vp, _vp, _vp, _vp]),
    "fovpt_temporal_reset": (_i32, [_vp]),
    "fovpt_temporal_gbuffer": (_i32, [_vp, _gbuf]),
    "fovpt_post_defaults": (_i32, [_P(abi.PostConfig)]),
    "fovpt_post": (_i32, [_vp, _params, _P(abi.PostConfig), _vp, _vp, _vp, _vp]),
    "fovpt_post_buffers": (_i32, _own2),
    "fovpt_expose_defaults": (_i32, [_P(abi.ExposeConfig)]),
    "fovpt_expose": (_i32, [_vp, _params, _P(abi.ExposeConfig), _vp, _vp, _vp]),
    "fovpt_expose_buffers": (_i32, _own2),
    "fovpt_expose_state": (_i32, [_vp, _P(abi.ExposeState)]),
    "fovpt_expose_reset": (_i32, [_vp]),
    "fovpt_bloom_defaults": (_i32, [_P(abi.BloomConfig)]),
    "fovpt_bloom": (_i32, [_vp, _params, _P(abi.BloomConfig), _vp, _vp, _vp]),
    "fovpt_bloom_buffers": (_i32, _own2),
    "fovpt_warp_defaults": (_i32, [_P(abi.WarpConfig)]),
    "fovpt_warp": (_i32, [_vp, _params, _cam, _P(abi.WarpConfig), _gbuf, _vp, _vp, _vp, _vp, _vp]),
    "fovpt_warp_buffers": (_i32, _own2),
    "fovpt_warp_counts": (_i32, [_vp, _P(abi.WarpCounts)]),
    "fovpt_warp_motion_defaults": (_i32, [_P(abi.WarpMotionConfig)]),
    "fovpt_warp_motion": (_i32, [_vp, _params, _cam, _P(abi.WarpMotionConfig), _gbuf, _vp, _vp, _vp, _vp, _vp]),
    "fovpt_focus_defaults": (_i32, [_P(abi.FocusConfig)]),
    "fovpt_focus": (_i32, [_vp, _params, _P(abi.FocusConfig), _gbuf, _vp, _vp, _vp, _vp]),
    "fovpt_focus_buffers": (_i32, _own2),
    "fovpt_focus_state": (_i32, [_vp, _P(abi.FocusState)]),
    "fovpt_focus_reset": (_i32, [_vp]),
    "fovpt_lens_defaults": (_i32, [_P(abi.LensConfig)]),
    "fovpt_lens": (_i32, [_vp, _params, _P(abi.LensConfig), _cam, _vp, _vp, _vp]),
    "fovpt_lens_buffers": (_i32, _own2),
    "fovpt_variance_defaults": (_i32, [_P(abi.VarianceConfig)]),
    "fovpt_variance": (_i32, [_vp, _params, _P(abi.VarianceConfig), _gbuf, _vp, _vp, _vp]),
    "fovpt_variance_buffers": (_i32, _own2),
    "fovpt_variance_reset": (_i32, [_vp]),
    "fovpt_variance_filter_defaults": (_i32, [_P(abi.VarianceFilterConfig)]),
    "fovpt_variance_filter": (_i32, [_vp, _params, _P(abi.VarianceFilterConfig), _gbuf, _vp, _vp, _vp, _vp]),
    "fovpt_variance_filter_buffers": (_i32, _own2),
    "fovpt_quality_defaults": (_i32, [_P(abi.QualityConfig)]),
    "fovpt_quality": (_i32, [_vp, _params, _P(abi.QualityConfig), _vp, _vp, _vp, _vp]),
    "fovpt_quality_read": (_i32, [_vp, _sums]),
    "fovpt_quality_host": (_i32, [_vp, _vp, _i32, _i32, _vp, C.c_int64, C.c_int64, _P(abi.QualityConfig), _sums]),
    "fovpt_quality_mse": (_f64, [_sums, _i32]),
    "fovpt_quality_psnr": (_f64, [_sums, _i32]),
    "fovpt_quality_ssim": (_f64, [_sums, _i32]),
    "fovpt_quality_score": (_f64, [_sums, _P(_f64)]),
    # -- frame packets (csrc/api_packet.hip, csrc/packet_host.cpp)
    "fovpt_packet_describe": (_i32, [_vp, _params, _u32, _P(abi.PacketHeader)]),
    "fovpt_packet_encode": (_i32, [_vp, _params, _vp, _u32, _vp]),
    "fovpt_packet_submit": (_i32, [_vp, _params, _vp, _u32, _P(_i32)]),
    "fovpt_packet_wait": (_i32, [_vp, _i32, _P(_vp), _P(_sz)]),
    "fovpt_packet_decode": (_i32, [_vp, _P(abi.PacketHeader), _vp, _i32, _vp]),
    "fovpt_packet_check": (_i32, [_vp, _sz]),
    "fovpt_packet_decode_host": (_i32, [_vp, _sz, _i32, _vp, _i32, _i32]),
    "fovpt_packet_defaults": (_i32, [_P(abi.PacketConfig)]),      # (void in the header; declared int here since it was added, the value is never read)
    "fovpt_packet_describe_coded": (_i32, [_vp, _params, _P(abi.PacketConfig), _u32, _P(abi.PacketHeader)]),
    "fovpt_packet_encode_coded": (_i32, [_vp, _params, _P(abi.PacketConfig), _vp, _u32, _vp]),
    "fovpt_packet_submit_coded": (_i32, [_vp, _params, _P(abi.PacketConfig), _vp, _u32, _P(_i32)]),
    # -- depth packets and the client's warp (csrc/api_packet.hip, csrc/packet_host.cpp, csrc/api_view.hip)
    "fovpt_packet_depth_defaults": (None, [_P(abi_depth.PacketDepthConfig)]),
    "fovpt_packet_describe_depth": (_i32, [_vp, _params, _P(abi_depth.PacketDepthConfig), _u32, _P(abi_depth.PacketDepthHeader)]),
    "fovpt_packet_encode_depth": (_i32, [_vp, _params, _P(abi_depth.PacketDepthConfig), _gbuf, _u32, _vp]),
    "fovpt_packet_submit_depth": (_i32, [_vp, _params, _P(abi_depth.PacketDepthConfig), _gbuf, _u32, _P(_i32)]),
    "fovpt_packet_check_depth": (_i32, [_vp, _sz]),
    "fovpt_packet_decode_depth_host": (_i32, [_vp, _sz, _vp, _i32, _i32]),
    "fovpt_packet_decode_depth": (_i32, [_vp, _P(abi_depth.PacketDepthHeader), _vp, _vp]),
    "fovpt_warp_depth": (_i32, [_vp, _i32, _i32, _cam, _cam, _P(abi.WarpConfig), _vp, _vp, _vp, _vp, _vp, _vp]),
    # -- animated geometry (csrc/api_animate.hip)
    "fovpt_update_vertices": (_i32, [_vp, _P(abi.VertexUpdate), _i32, _i32]),
    "fovpt_update_transforms": (_i32, [_vp, _P(abi.MeshTransform), _i32, _i32]),
    "fovpt_hierarchy_cost": (_i32, [_vp, _i32, _P(abi.HierarchyCost)]),
    "fovpt_rebuild_state": (_i32, [_vp, _i32, _P(abi.RebuildInfo)]),
    "fovpt_set_skins": (_i32, [_vp, _P(abi.MeshSkin), _i32]),
    "fovpt_update_skinned": (_i32, [_vp, _P(abi.SkinPose), _i32, _i32]),
    "fovpt_set_morphs": (_i32, [_vp, _P(abi.MeshMorph), _i32]),
    "fovpt_update_morphed": (_i32, [_vp, _P(abi.MorphPose), _i32, _i32]),
    "fovpt_set_rig": (_i32, [_vp, _P(abi.RigDesc)]),
    "fovpt_update_animated": (_i32, [_vp, _i32, _f32, _i32]),
    # -- test hooks (csrc/api_debug.hip)
    "fovpt_debug_math": (_i32, [_vp, _i32, _vp, _vp, _vp, _sz]),
    "fovpt_debug_buffer": (_i32, [_vp, _str, _P(_vp), _P(_sz)]),
    "fovpt_debug_trace": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "fovpt_debug_trace_queued": (_i32, [_vp, _P(abi.DebugTraceLaunch), _P(abi.DebugTraceResult)]),
    "fovpt_debug_probe_sample": (_i32, [_vp, _P(abi.Probe), _i32, _i32, _vp, _vp, _vp, _P(_i32)]),
    "fovpt_debug_probe_eval": (_i32, [_vp, _P(abi.Probe), _i32, _i32, _vp, _vp, _P(_i32)]),
    "fovpt_debug_bsdf": (_i32, [_vp, _P(abi.Material), _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fovpt_debug_tex2d": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "fovpt_debug_shade": (_i32, [_vp, _P(abi.Probe), _P(abi.DebugShadeLaunch), _vp, _vp, _vp, _vp, _vp, _vp, _P(abi.DebugShadeResult)]),
    "fovpt_debug_resolve": (_i32, [_vp, _params, _i32, _u32, _u32, _P(abi.DebugPass), _P(_i32), _vp, _vp, _vp, _vp, _vp, _vp, _P(_u32)]),
    "fovpt_debug_generate": (_i32, [_vp, _params, _P(abi.DebugGenerateLaunch), _P(abi.DebugPass), _P(_i32), _P(abi.DebugGenerateResult)]),
    "fovpt_debug_build": (_i32, [_vp, _u32, _vp, _vp, _P(abi.DebugBuildSwitches), _P(abi.DebugBuildTrace)]),
    # -- scene and image files (csrc/model_loader.cpp)
    "fovpt_model_load_obj": (_i32, [_str, _P(_vp)]),
    "fovpt_model_load_gltf": (_i32, [_str, _P(_vp)]),
    "fovpt_model_destroy": (None, [_vp]),
    "fovpt_model_counts": (_i32, [_vp, _P(_i32), _P(_i32)]),
    "fovpt_model_get_mesh": (_i32, [_vp, _i32, _P(abi.ModelMesh)]),
    "fovpt_model_get_texture": (_i32, [_vp, _i32, _P(_vp), _P(_i32), _P(_i32)]),
    "fovpt_image_load_float4": (_i32, [_str, _P(_i32), _P(_i32), _P(_vp)]),
    "fovpt_image_free": (None, [_vp]),
    "fovpt_image_load_rgba8": (_i32, [_str, _P(_i32), _P(_i32), _P(_vp)]),
    "fovpt_image_free_rgba8": (None, [_vp]),
}

EXPORTS = list(SIGNATURES)
# what the host-only libfovpt_loader.so has too (load_loader): the file readers, the packet checks and decoder for a client
# (csrc/packet_host.cpp), the quality measurement on host images and the scores of a record (csrc/quality_host.cpp)
LOADER_EXPORTS = [n for n in EXPORTS if n.startswith("fovpt_model_") or n.startswith("fovpt_image_")] + ["fovpt_last_error"]
PACKET_HOST_EXPORTS = ["fovpt_packet_check", "fovpt_packet_decode_host", "fovpt_packet_depth_defaults", "fovpt_packet_check_depth",
                       "fovpt_packet_decode_depth_host"]
QUALITY_SCORE_EXPORTS = ("fovpt_quality_mse", "fovpt_quality_psnr", "fovpt_quality_ssim", "fovpt_quality_score")   # return a double
QUALITY_HOST_EXPORTS = ["fovpt_quality_host"] + list(QUALITY_SCORE_EXPORTS)
LOADER_SO_PATH = os.path.join(CSRC, "libfovpt_loader.so")


def declare(L, names=EXPORTS):
    """Gives the functions `names` of the loaded library L the restype and argtypes of their SIGNATURES rows."""
    for name in names:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = SIGNATURES[name]
    return L


def _declare_loader(L):
    """declare() for the rows both libraries share: what a caller that opened libfovpt_loader.so itself applies (the packet tests do)."""
    declare(L, LOADER_EXPORTS)


def _declare_packet_host(L):
    """The same for the packet checks and the decoder for a client."""
    declare(L, PACKET_HOST_EXPORTS)


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


def _torch_lib(name, *skip_env):
    """The path of torch's bundled lib/<name> when torch is installed but not imported yet and none of skip_env is set; else None."""
    import importlib.util
    import sys
    if "torch" in sys.modules or any(os.environ.get(k) for k in skip_env):
        return None
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return None
    if spec is None or not spec.submodule_search_locations:
        return None
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", name)
    return path if os.path.exists(path) else None


def _share_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's, found by file name
    through an RPATH).  Imported FIRST, torch's copy also serves libfovpt.so; imported AFTER libfovpt.so has
    pulled in /opt/rocm's copy, torch loads a second HIP/HSA runtime into the process, which finds "No HIP
    GPUs".  So when torch is installed but not imported yet, its copy is loaded here, and either import order
    ends with one runtime.  Without torch (C++ callers, plain Python) the library binds to /opt/rocm as linked.
    FOVPT_SYSTEM_HIP=1 skips this."""
    hip = _torch_lib("libamdhip64.so", "FOVPT_SYSTEM_HIP")
    if hip:
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
    rccl = _torch_lib("librccl.so", "FOVPT_SYSTEM_HIP", "FOVPT_RCCL_LIB")
    if rccl:
        try:
            C.CDLL(rccl)
        except OSError:
            pass


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise FovptError(-100, "%s is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)" % SO_PATH)
    _share_torch_hip_runtime()
    _lib = declare(C.CDLL(SO_PATH))
    return _lib


_loader = None


def load_loader():
    """The scene / image ingestion of the C ABI (fovpt_model_*, fovpt_image_*), the packet decoder for a client
    (PACKET_HOST_EXPORTS) and the quality measurement on host images (QUALITY_HOST_EXPORTS).  If libfovpt.so is already loaded, it; otherwise the
    HOST-ONLY libfovpt_loader.so (same code, g++, no HIP runtime), so that reading OBJ / glTF / JPEG / HDR files needs no GPU
    stack; FOVPT_SO (an A/B build of the whole library) takes precedence.  The render path never goes through here."""
    global _loader
    if _lib is not None or os.environ.get("FOVPT_SO") or not os.path.exists(LOADER_SO_PATH):
        return load()
    if _loader is None:
        _loader = declare(C.CDLL(LOADER_SO_PATH), LOADER_EXPORTS + PACKET_HOST_EXPORTS + QUALITY_HOST_EXPORTS)
    return _loader


def check(ctx, rc, L=None):
    """Raises FovptError with the library's text; `L`: the library the failing call was made in (the loader library keeps its own
    error text)."""
    if rc != 0:
        msg = (L or load()).fovpt_last_error(ctx)
        raise FovptError(rc, msg.decode("utf-8", "replace") if msg else "")
