"""ctypes mirror of include/fovpt.h (the C ABI of libfovpt).

Layouts follow the reference's device-visible structs: Material (PT_sv5_/Material.h:48-69),
Probe (PT_sv5_/Probe.cuh:6-21), LaunchParams (PT_sv5_/LaunchParams.h:49-91).
"""
import ctypes as C

FOVPT_OK = 0
MATERIAL_FLAG_SHADOW_CATCHER = 1
OPT_SKY_MISS, OPT_RUSSIAN_ROULETTE = 1, 2      # fovpt_config.options (include/fovpt.h)

OP_SIN, OP_COS, OP_ACOS, OP_ATAN2, OP_LOG, OP_POW, OP_SQRT, OP_DIV, OP_RSQRTD, OP_UNORM8, OP_HALFPLUS = range(1, 12)


class Struct(C.Structure):
    """What every mirror below shares (no _fields_ of its own, no C counterpart)."""

    def copy(self):
        """A new object of the same class with the same bytes."""
        m = type(self)()
        C.memmove(C.byref(m), C.byref(self), C.sizeof(self))
        return m

    def as_dict(self):
        """The public fields (names that do not start with "_"); arrays as tuples."""
        out = {}
        for n, _ in self._fields_:
            if not n.startswith("_"):
                v = getattr(self, n)
                out[n] = tuple(v) if isinstance(v, C.Array) else v
        return out


class Float3(Struct):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]

    def set(self, v):
        self.x, self.y, self.z = float(v[0]), float(v[1]), float(v[2])
        return self

    def tolist(self):
        return [self.x, self.y, self.z]


class Float4(Struct):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("w", C.c_float)]


class Int2(Struct):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32)]


class UInt2(Struct):
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32)]


class UInt3(Struct):
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("z", C.c_uint32)]


class Material(Struct):
    """fovpt_material == Material (PT_sv5_/Material.h).  Construct with Material.reference_default()
    to get the non-trivial constructor defaults of Material.h:13-38."""
    _fields_ = [
        ("emission", Float3), ("color", Float3), ("absorption", Float3),
        ("eta", C.c_float), ("metallic", C.c_float), ("subsurface", C.c_float),
        ("specular", C.c_float), ("roughness", C.c_float), ("specularTint", C.c_float),
        ("anisotropic", C.c_float), ("sheen", C.c_float), ("sheenTint", C.c_float),
        ("clearcoat", C.c_float), ("clearcoatGloss", C.c_float), ("transmission", C.c_float),
        ("bump", C.c_float), ("bumpTile", Float3), ("flags", C.c_int32),
    ]

    @classmethod
    def reference_default(cls):
        m = cls()
        m.color.set((1.0, 0.0, 0.0))
        m.emission.set((1.0, 1.0, 1.0))
        m.absorption.set((1.0, 1.0, 1.0))
        m.eta = 1.4
        m.metallic = 0.5
        m.subsurface = 0.0
        m.specular = 1.0
        m.roughness = 1.0
        m.specularTint = 1.0
        m.anisotropic = 0.0
        m.sheen = 0.0
        m.sheenTint = 0.0
        m.clearcoat = 0.0
        m.clearcoatGloss = 1.0
        m.transmission = 0.4
        m.bump = 0.0
        m.bumpTile.set((1.0, 1.0, 1.0))
        m.flags = 0
        return m


class Probe(Struct):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("data", C.c_void_p),
        ("offset", Float3), ("_pad0", C.c_uint32),
        ("pdfValuesX", C.c_void_p), ("cdfValuesX", C.c_void_p),
        ("pdfValuesY", C.c_void_p), ("cdfValuesY", C.c_void_p),
    ]


class _Frame(Struct):
    _fields_ = [
        ("accum_buffer", C.c_void_p), ("frame_buffer", C.c_void_p),
        ("color_buffer", C.c_void_p), ("normal_buffer", C.c_void_p), ("albedo_buffer", C.c_void_p),
        ("size", Int2), ("subframe_index", C.c_uint32), ("factor", UInt3),
        ("fillSize", C.c_int32), ("_pad0", C.c_uint32), ("c", UInt2),
        ("r_inner", C.c_float), ("r_outer", C.c_float), ("offset", UInt2),
        ("redraw", C.c_uint32), ("_pad1", C.c_uint32),
    ]


class _Camera(Struct):
    _fields_ = [("eye", Float3), ("U", Float3), ("V", Float3), ("W", Float3)]


class LaunchParams(Struct):
    _fields_ = [
        ("frame", _Frame), ("camera", _Camera),
        ("samples_per_launch", C.c_uint32), ("_pad2", C.c_uint32),
        ("traversable", C.c_uint64), ("probe", Probe),
        ("viewportSize", Int2), ("white", C.c_float), ("_pad3", C.c_uint32),
    ]


class MeshDesc(Struct):
    _fields_ = [
        ("vertex", C.c_void_p), ("normal", C.c_void_p), ("texcoord", C.c_void_p), ("index", C.c_void_p),
        ("num_vertices", C.c_uint32), ("num_triangles", C.c_uint32),
        ("texture_id", C.c_int32), ("material", Material),
    ]


class ModelMesh(Struct):
    """fovpt_model_mesh: one TriangleMesh of a model loaded by fovpt_model_load_obj (arrays owned by the model)."""
    _fields_ = [
        ("vertex", C.c_void_p), ("normal", C.c_void_p), ("texcoord", C.c_void_p), ("index", C.c_void_p),
        ("num_vertices", C.c_uint32), ("num_normals", C.c_uint32), ("num_texcoords", C.c_uint32), ("num_triangles", C.c_uint32),
        ("material", Material), ("diffuse_texture_id", C.c_int32),
    ]


UPDATE_DEVICE, UPDATE_REBUILD = 1, 2            # fovpt_update_vertices flags (FOVPT_UPDATE_*)
UPDATE_REBUILD_ASYNC = 16                       # FOVPT_UPDATE_REBUILD_ASYNC: all five fovpt_update_* calls
REBUILD_IDLE, REBUILD_BUILDING, REBUILD_READY = 0, 1, 2     # fovpt_rebuild_info.state (FOVPT_REBUILD_*)
REBUILD_WAIT, REBUILD_ADOPT = 1, 2              # fovpt_rebuild_state flags


class VertexUpdate(Struct):
    """fovpt_vertex_update: new xyz positions for one mesh of the scene (host, or device with UPDATE_DEVICE)."""
    _fields_ = [("mesh", C.c_int32), ("num_vertices", C.c_uint32), ("vertex", C.c_void_p)]


class MeshTransform(Struct):
    """fovpt_mesh_transform: a row-major 3 x 4 matrix applied to the rest positions of one mesh (fovpt_update_transforms)."""
    _fields_ = [("mesh", C.c_int32), ("m", C.c_float * 12)]


DEBUG_PROBE_PLAIN = 1                           # fovpt_debug_probe_sample / _probe_eval flag (FOVPT_DEBUG_PROBE_PLAIN)
PROBE_PATH_GUIDED, PROBE_PATH_RECORDS, PROBE_PATH_ONE_ROW = 1, 2, 4   # their *path_out bits (FOVPT_PROBE_PATH_*)
COST_WAIT = 1                                   # fovpt_hierarchy_cost flag (FOVPT_COST_WAIT)
STATE_DONE, STATE_SECONDARY, STATE_ALPHA_ONE, STATE_ALPHA_SET = 1, 2, 4, 8   # a sample slot's flags, below depth << 8 (fovpt_debug_resolve)


class DebugPass(Struct):
    """struct fovpt_debug_pass: one pass of the frame fovpt_debug_resolve resolves, and its place in the caller's arrays."""
    _fields_ = [("gw", C.c_uint32), ("rows", C.c_uint32), ("spp", C.c_uint32), ("slot_base", C.c_uint32), ("launch_base", C.c_uint32)]


DEBUG_SHADE_FILL = 0xcd                         # FOVPT_DEBUG_SHADE_FILL: the byte fovpt_debug_shade fills every output buffer with


class DebugShadeLaunch(Struct):
    """struct fovpt_debug_shade_launch."""
    _fields_ = [("n", C.c_int32), ("depth_iter", C.c_int32), ("grid", C.c_int32), ("partition", C.c_int32), ("sel", C.c_uint32),
                ("shard_count", C.c_uint32 * 8)]


class DebugShadeResult(Struct):
    """struct fovpt_debug_shade_result: host arrays of the caller's, and what the call counted."""
    _fields_ = [(k, C.c_void_p) for k in ("rng4", "thr4", "rad4", "alpha4", "guide_n4", "guide_a4", "next_place2", "next_o4", "next_d4",
                                          "shadow_place2", "shadow_o4", "shadow_d4", "shadow_vis4", "shadow_occ4")] + [
        ("next_count", C.c_uint32 * 8), ("shadow_count", C.c_uint32 * 8),
        ("next_found", C.c_uint32), ("shadow_found", C.c_uint32), ("counters_changed", C.c_uint32), ("cap", C.c_uint32)]


DEBUG_TRACE_ALPHA = 0xffffffff                  # FOVPT_DEBUG_TRACE_ALPHA: a shadow record whose target is the slot's alpha
DEBUG_TRACE_ITERS = 63                          # FOVPT_DEBUG_TRACE_ITERS: the iterations fovpt_debug_trace_queued may name


class DebugTraceLaunch(Struct):
    """struct fovpt_debug_trace_launch: host arrays of the caller's for the two ray sets, and the launch."""
    _fields_ = [(k, C.c_void_p) for k in ("origins3", "dirs3", "slot", "target", "vis4", "occ4", "other_origins3", "other_dirs3", "other_slot",
                                          "other_target", "other_vis4", "other_occ4")] + [
        ("n", C.c_int32), ("n_other", C.c_int32), ("sel", C.c_uint32), ("both", C.c_uint32), ("it_closest", C.c_int32), ("it_shadow", C.c_int32),
        ("grid_closest", C.c_int32), ("grid_shadow", C.c_int32), ("slots", C.c_uint32), ("q_count", C.c_uint32 * 8), ("sq_count", C.c_uint32 * 8),
        ("other_q_count", C.c_uint32 * 8), ("other_sq_count", C.c_uint32 * 8), ("decoy", C.c_uint32 * 8)]


class DebugTraceResult(Struct):
    """struct fovpt_debug_trace_result: host arrays of the caller's, and what the call counted."""
    _fields_ = [(k, C.c_void_p) for k in ("hit_place2", "hit4", "hit_prim", "cells4", "alpha4")] + [
        ("stat_radiance", C.c_uint64), ("stat_shadow", C.c_uint64), ("stat_paths", C.c_uint64),
        ("hit_found", C.c_uint32), ("counters_changed", C.c_uint32), ("queues_unchanged", C.c_uint32), ("cap", C.c_uint32)]


class DebugGenerateLaunch(Struct):
    """struct fovpt_debug_generate_launch."""
    _fields_ = [("render", C.c_int32), ("width", C.c_uint32), ("height", C.c_uint32), ("row0", C.c_uint32), ("row1", C.c_uint32),
                ("sel", C.c_uint32), ("slot_begin", C.c_uint32), ("slot_end", C.c_uint32), ("grid", C.c_int32)]


class DebugGenerateResult(Struct):
    """struct fovpt_debug_generate_result: host arrays of the caller's, and what the call counted."""
    _fields_ = [(k, C.c_void_p) for k in ("rng4", "backplate4", "guide_n4", "guide_a4", "place2", "o4", "d4")] + [
        ("count", C.c_uint32 * 8), ("found", C.c_uint32), ("counters_changed", C.c_uint32), ("cap", C.c_uint32), ("kernel", C.c_uint32),
        ("guides", C.c_uint32), ("slot_begin", C.c_uint32), ("slot_end", C.c_uint32), ("grid", C.c_uint32)]


class DebugBuildSwitches(Struct):
    """struct fovpt_debug_build_switches: the switches of one fovpt_debug_build, nothing from the environment."""
    _fields_ = [("use_ploc", C.c_int32), ("split_budget", C.c_float), ("reinsert_rounds", C.c_int32), ("order_children", C.c_int32)]


class DebugBuildTrace(Struct):
    """struct fovpt_debug_build_trace: host arrays of the caller's for what every stage of a build left, and its scalars."""
    _fields_ = [(k, C.c_void_p) for k in ("split_count", "split_first", "ref_prim", "boxes", "keys_s", "vals_s", "left0", "right0", "ibox0",
                                          "round_end", "left1", "right1", "ibox1", "size_int", "node_first", "leaf_pos", "dp", "nodes_pre",
                                          "nodes", "tris")] + [
        (k, C.c_uint32) for k in ("cap_refs", "cap_rounds", "num_refs", "tiny", "have_count", "have_splits", "root", "num_rounds", "num_nodes",
                                  "max_depth", "reinserted", "num_levels")] + [
        ("s_cut", C.c_float), ("cbounds", C.c_float * 6), ("level_first", C.c_uint32 * 65)]


class HierarchyCost(Struct):
    """fovpt_hierarchy_cost_info: the SAH cost of the hierarchy as built and as last measured, and the update counters."""
    _fields_ = [("built", C.c_double), ("current", C.c_double), ("updates", C.c_uint64), ("measured", C.c_uint64)]


class RebuildInfo(Struct):
    """fovpt_rebuild_info: the state of the background rebuild (FOVPT_UPDATE_REBUILD_ASYNC) and its counters."""
    _fields_ = [("state", C.c_int32), ("last_error", C.c_int32), ("requested", C.c_uint64), ("started", C.c_uint64), ("adopted", C.c_uint64),
                ("failed", C.c_uint64), ("discarded", C.c_uint64), ("snapshot_update", C.c_uint64), ("ms_build", C.c_double)]


SKIN_MAX_JOINTS = 1024                          # FOVPT_SKIN_MAX_JOINTS


class MeshSkin(Struct):
    """fovpt_mesh_skin: four joint indices and four weights per vertex of one mesh (fovpt_set_skins); num_joints 0 and two null
    pointers remove the mesh's skin."""
    _fields_ = [("mesh", C.c_int32), ("num_vertices", C.c_uint32), ("num_joints", C.c_uint32), ("_reserved", C.c_uint32),
                ("joints", C.c_void_p), ("weights", C.c_void_p)]


class SkinPose(Struct):
    """fovpt_skin_pose: the palette of one skinned mesh, num_joints row-major 3 x 4 matrices (fovpt_update_skinned)."""
    _fields_ = [("mesh", C.c_int32), ("num_joints", C.c_uint32), ("matrices", C.c_void_p)]


MORPH_MAX_TARGETS = 256                         # FOVPT_MORPH_MAX_TARGETS


class MorphTarget(Struct):
    """fovpt_morph_target: the vertices one target moves and their deltas; index null: dense, entry i is vertex i."""
    _fields_ = [("count", C.c_uint32), ("_reserved", C.c_uint32), ("index", C.c_void_p), ("delta", C.c_void_p)]


class MeshMorph(Struct):
    """fovpt_mesh_morph: the morph targets of one mesh (fovpt_set_morphs); num_targets 0 and a null pointer remove them."""
    _fields_ = [("mesh", C.c_int32), ("num_vertices", C.c_uint32), ("num_targets", C.c_uint32), ("_reserved", C.c_uint32),
                ("targets", C.POINTER(MorphTarget))]


class MorphPose(Struct):
    """fovpt_morph_pose: one weight per target of a morphed mesh and, with num_joints > 0, its skin's palette
    (fovpt_update_morphed)."""
    _fields_ = [("mesh", C.c_int32), ("num_targets", C.c_uint32), ("weights", C.c_void_p), ("num_joints", C.c_uint32),
                ("_reserved", C.c_uint32), ("matrices", C.c_void_p)]


RIG_MAX_NODES, RIG_MAX_CLIPS, RIG_MAX_KEYS = 1024, 64, 1 << 20           # FOVPT_RIG_MAX_NODES / _CLIPS / _KEYS
RIG_TRANSLATION, RIG_ROTATION, RIG_SCALE, RIG_WEIGHTS = 0, 1, 2, 3        # FOVPT_RIG_TRANSLATION ..: a channel's path
RIG_STEP, RIG_LINEAR = 0, 1                                               # FOVPT_RIG_STEP / _LINEAR: its interpolation


class RigNode(Struct):
    """fovpt_rig_node: a node's parent (-1: a root; otherwise below its own index) and rest pose, rotation as x y z w."""
    _fields_ = [("parent", C.c_int32), ("translation", C.c_float * 3), ("rotation", C.c_float * 4), ("scale", C.c_float * 3)]


class RigBinding(Struct):
    """fovpt_rig_binding: one mesh the rig drives: rigidly by a node, through its skin by joint nodes and inverse bind matrices,
    or (node -1, no joints) by morph weights alone."""
    _fields_ = [("mesh", C.c_int32), ("node", C.c_int32), ("num_joints", C.c_uint32), ("_reserved", C.c_uint32),
                ("joint_nodes", C.c_void_p), ("inverse_bind", C.c_void_p)]


class RigChannel(Struct):
    """fovpt_rig_channel: the keys of one path of one node (WEIGHTS: of one mesh)."""
    _fields_ = [("target", C.c_int32), ("path", C.c_int32), ("interpolation", C.c_int32), ("num_keys", C.c_uint32),
                ("times", C.c_void_p), ("values", C.c_void_p)]


class RigClip(Struct):
    """fovpt_rig_clip: the channels of one clip."""
    _fields_ = [("num_channels", C.c_uint32), ("_reserved", C.c_uint32), ("channels", C.POINTER(RigChannel))]


class RigDesc(Struct):
    """fovpt_rig_desc: nodes, bindings and clips (fovpt_set_rig)."""
    _fields_ = [("nodes", C.POINTER(RigNode)), ("num_nodes", C.c_uint32), ("_reserved0", C.c_uint32),
                ("bindings", C.POINTER(RigBinding)), ("num_bindings", C.c_uint32), ("_reserved1", C.c_uint32),
                ("clips", C.POINTER(RigClip)), ("num_clips", C.c_uint32), ("_reserved2", C.c_uint32)]


class TextureDesc(Struct):
    _fields_ = [("pixel", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32)]


class Config(Struct):
    _fields_ = [
        ("uniform", C.c_int32), ("r_inner", C.c_int32), ("r_outer", C.c_int32),
        ("spp_periphery", C.c_int32), ("spp_middle", C.c_int32), ("spp_fovea", C.c_int32),
        ("spp_uniform", C.c_int32), ("max_depth", C.c_int32), ("accumulate", C.c_int32),
        ("rank", C.c_int32), ("world", C.c_int32), ("tile_w", C.c_int32), ("tile_h", C.c_int32),
        ("profile", C.c_int32), ("write_guides", C.c_int32), ("options", C.c_int32),
        ("frames_in_flight", C.c_int32),      # 0 = library default (2), 1, 2
        ("chains_per_frame", C.c_int32),      # 0 / 1 = one chain per frame, 2 = two (for callers that synchronise every frame)
    ]

    @classmethod
    def reference_default(cls):
        """PT_sv5_ as shipped: FOV_ON, radii 74/241, spp 8/16/32, uniform spp 4, depth cap 4."""
        c = cls()
        c.uniform = 0
        c.r_inner, c.r_outer = 74, 241
        c.spp_periphery, c.spp_middle, c.spp_fovea, c.spp_uniform = 8, 16, 32, 4
        c.max_depth = 4
        c.accumulate = 0
        c.rank, c.world = 0, 1
        c.tile_w, c.tile_h = 8, 4
        return c


DENOISE_MAX_ITERATIONS = 5                     # FOVPT_DENOISE_MAX_ITERATIONS
SIGMA_MIN, SIGMA_MAX = 1e-6, 1e6               # FOVPT_SIGMA_MIN / MAX (binary32 1e-6f / 1e6f): accepted *_sigma of both configs


class DenoiseConfig(Struct):
    """fovpt_denoise_config: iterations per foveation level and the edge-stopping scales (defaults: fovpt_denoise_defaults)."""
    _fields_ = [
        ("iterations_fovea", C.c_int32), ("iterations_middle", C.c_int32), ("iterations_periphery", C.c_int32),
        ("iterations_uniform", C.c_int32),
        ("color_sigma", C.c_float), ("normal_sigma", C.c_float), ("albedo_sigma", C.c_float),
        ("_reserved", C.c_int32),
    ]


class ReconstructConfig(Struct):
    """fovpt_reconstruct_config: tent support, edge-stopping scales, levels and remodulation (defaults: fovpt_reconstruct_defaults)."""
    _fields_ = [
        ("support", C.c_float), ("normal_sigma", C.c_float), ("depth_sigma", C.c_float),
        ("levels", C.c_int32), ("remodulate", C.c_int32),
        ("_reserved", C.c_int32 * 3),
    ]


class GBufferPtrs(Struct):
    """fovpt_gbuffer_ptrs: device pointers of the G-buffer fovpt_gbuffer filled."""
    _fields_ = [
        ("prim", C.c_void_p), ("position", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p),
        ("width", C.c_int32), ("height", C.c_int32),
    ]


TEMPORAL_MAX_HISTORY = 64                      # FOVPT_TEMPORAL_MAX_HISTORY


class TemporalConfig(Struct):
    """fovpt_temporal_config: history caps per foveation level and the reprojection tolerances (defaults: fovpt_temporal_defaults)."""
    _fields_ = [
        ("history_fovea", C.c_int32), ("history_middle", C.c_int32), ("history_periphery", C.c_int32),
        ("history_uniform", C.c_int32),
        ("normal_tolerance", C.c_float), ("depth_tolerance", C.c_float),
        ("_reserved", C.c_int32 * 2),
    ]


POST_DENOISE, POST_RECONSTRUCT, POST_TEMPORAL, POST_MOTION = 1, 2, 4, 8     # FOVPT_POST_*


class PostConfig(Struct):
    """fovpt_post_config: the stages of the post-frame chain (POST_* bits) and each stage's own config (defaults: fovpt_post_defaults)."""
    _fields_ = [
        ("stages", C.c_int32),
        ("_reserved", C.c_int32 * 3),
        ("denoise", DenoiseConfig), ("reconstruct", ReconstructConfig), ("temporal", TemporalConfig),
    ]


EXPOSE_FIXED, EXPOSE_AUTO = 0, 1               # FOVPT_EXPOSE_*
METER_FRAME, METER_GAZE = 0, 1                 # FOVPT_METER_*
TONE_REINHARD, TONE_ACES = 0, 1                # FOVPT_TONE_*
EXPOSE_BINS = 256                              # FOVPT_EXPOSE_BINS


class ExposeConfig(Struct):
    """fovpt_expose_config: mode, metering, tone map, the meter's weights per foveation level and its trimmed mean, the key and
    the adaptation rates (defaults: fovpt_expose_defaults)."""
    _fields_ = [
        ("mode", C.c_int32), ("metering", C.c_int32), ("tone", C.c_int32), ("_reserved0", C.c_int32),
        ("weight_fovea", C.c_int32), ("weight_middle", C.c_int32), ("weight_periphery", C.c_int32), ("weight_uniform", C.c_int32),
        ("low_permille", C.c_int32), ("high_permille", C.c_int32),
        ("ev_min", C.c_float), ("ev_max", C.c_float),
        ("key", C.c_float), ("exposure", C.c_float), ("white", C.c_float),
        ("adapt_brighter", C.c_float), ("adapt_darker", C.c_float),
        ("_reserved", C.c_int32 * 3),
    ]


class ExposeState(Struct):
    """struct fovpt_expose_state: the metered and the adapted log2 luminance, the exposure, the last meter's total weight and the
    AUTO steps since create / reset."""
    _fields_ = [
        ("ev_metered", C.c_float), ("ev", C.c_float), ("exposure", C.c_float), ("_pad", C.c_float),
        ("weight_total", C.c_uint64), ("steps", C.c_uint64),
    ]


BLOOM_MAX_LEVELS = 8                           # FOVPT_BLOOM_MAX_LEVELS
BLOOM_KARIS, BLOOM_GAINS, BLOOM_EXPOSURE_STATE = 1, 2, 4     # FOVPT_BLOOM_* (flags)


class BloomConfig(Struct):
    """fovpt_bloom_config: flags, levels, the threshold and knee in exposed units, the exposure they are divided by, the intensity
    of the composite, the spread between levels and the gains per foveation level (defaults: fovpt_bloom_defaults)."""
    _fields_ = [
        ("flags", C.c_int32), ("levels", C.c_int32),
        ("threshold", C.c_float), ("knee", C.c_float), ("exposure", C.c_float),
        ("intensity", C.c_float), ("spread", C.c_float),
        ("gain_fovea", C.c_float), ("gain_middle", C.c_float), ("gain_periphery", C.c_float), ("gain_uniform", C.c_float),
        ("_reserved", C.c_int32 * 5),
    ]


WARP_COLOR, WARP_RGBA = 1, 2                   # FOVPT_WARP_*
WARP_MAX_RADIUS = 4                            # FOVPT_WARP_MAX_RADIUS
WARP_DIRECT, WARP_FILLED, WARP_EMPTY = 0, 1, 2  # the class in bits 30 .. 31 of a warp map entry


class WarpCamera(Struct):
    """fovpt_warp_camera: the camera fovpt_warp re-aims the frame at, in LaunchParams.camera's layout."""
    _fields_ = [("eye", Float3), ("U", Float3), ("V", Float3), ("W", Float3)]


class WarpConfig(Struct):
    """fovpt_warp_config: the images to warp (WARP_* bits) and the radius of the hole fill (defaults: fovpt_warp_defaults)."""
    _fields_ = [("images", C.c_int32), ("fill_radius", C.c_int32), ("_reserved", C.c_int32 * 6)]


WARP_MAX_ADVANCE = 4.0                         # FOVPT_WARP_MAX_ADVANCE


class WarpMotionConfig(Struct):
    """fovpt_warp_motion_config: WarpConfig's images and fill radius, and how far past the rendered frame the moved meshes are
    extrapolated, in intervals between the last two temporal steps (defaults: fovpt_warp_motion_defaults)."""
    _fields_ = [("images", C.c_int32), ("fill_radius", C.c_int32), ("advance", C.c_float), ("_reserved", C.c_int32 * 5)]


class WarpCounts(Struct):
    """struct fovpt_warp_counts: the source pixels of the last warp that landed in the frame, and its destination pixels by class."""
    _fields_ = [("splatted", C.c_uint64), ("direct", C.c_uint64), ("filled", C.c_uint64), ("empty", C.c_uint64)]


FOCUS_FIXED, FOCUS_AUTO = 0, 1                 # FOVPT_FOCUS_*
FOCUS_MAX_RADIUS, FOCUS_MAX_METER_RADIUS, FOCUS_BINS = 8, 64, 256


class FocusConfig(Struct):
    """fovpt_focus_config: mode, the gaze disc and rank of the meter, the blur's cap and strength, the fixed and the default focus
    distance and the adaptation rates (defaults: fovpt_focus_defaults)."""
    _fields_ = [
        ("mode", C.c_int32), ("meter_radius", C.c_int32), ("rank_permille", C.c_int32), ("max_radius", C.c_int32),
        ("strength", C.c_float), ("focus_distance", C.c_float), ("focus_default", C.c_float),
        ("adapt_nearer", C.c_float), ("adapt_farther", C.c_float),
        ("_reserved", C.c_int32 * 7),
    ]


class FocusState(Struct):
    """struct fovpt_focus_state: the metered distance, the adapted reciprocal distance and distance, the pixels the last meter
    counted and the AUTO steps since create / reset."""
    _fields_ = [
        ("focus_metered", C.c_float), ("inv_focus", C.c_float), ("focus", C.c_float), ("_pad", C.c_float),
        ("count", C.c_uint64), ("steps", C.c_uint64),
    ]


LENS_NEAREST, LENS_BILINEAR, LENS_BICUBIC = 0, 1, 2    # FOVPT_LENS_*
LENS_ENCODE_DISPLAY, LENS_ENCODE_RESOLVE = 0, 1


class LensConfig(Struct):
    """fovpt_lens_config: the filter and the rgba8 encoding, the lens axis and scale in destination NDC, the radial polynomial and
    its per-channel factors, the lens's clip radius, the map from lens units to source NDC and the border colour (defaults:
    fovpt_lens_defaults)."""
    _fields_ = [
        ("filter", C.c_int32), ("encode", C.c_int32), ("_reserved0", C.c_int32 * 2),
        ("center", C.c_float * 2), ("scale", C.c_float * 2), ("k", C.c_float * 4), ("chroma", C.c_float * 3), ("clip_r2", C.c_float),
        ("src_center", C.c_float * 2), ("src_scale", C.c_float * 2), ("border", C.c_float * 4),
        ("_reserved", C.c_int32 * 8),
    ]


class VarianceConfig(Struct):
    """fovpt_variance_config: the cap of the moment history, the history length below which the spatial estimate is taken, that
    estimate's radius and the tolerances of the history taps and the window (defaults: fovpt_variance_defaults)."""
    _fields_ = [
        ("history_cap", C.c_int32), ("spatial_below", C.c_int32), ("spatial_radius", C.c_int32),
        ("depth_tolerance", C.c_float), ("normal_tolerance", C.c_float),
        ("_reserved", C.c_int32 * 3),
    ]


class VarianceFilterConfig(Struct):
    """fovpt_variance_filter_config: a-trous iterations per foveation level, the luminance (in standard deviations), normal and
    plane-distance edge-stopping scales and the albedo demodulation (defaults: fovpt_variance_filter_defaults)."""
    _fields_ = [
        ("iterations_fovea", C.c_int32), ("iterations_middle", C.c_int32), ("iterations_periphery", C.c_int32), ("iterations_uniform", C.c_int32),
        ("luminance_sigma", C.c_float), ("normal_sigma", C.c_float), ("depth_sigma", C.c_float),
        ("demodulate", C.c_int32),
        ("_reserved", C.c_int32 * 4),
    ]


QUALITY_SSIM, QUALITY_PROFILE = 1, 2                   # FOVPT_QUALITY_* flags
QUALITY_CLASSES, QUALITY_RINGS, QUALITY_MAX_RING_WIDTH = 5, 64, 65536
QUALITY_FOVEA, QUALITY_MIDDLE, QUALITY_PERIPHERY, QUALITY_UNIFORM, QUALITY_UNWRITTEN = 0, 1, 2, 3, 4   # a pixel's class
QUALITY_CLASS_NAMES = ("fovea", "middle", "periphery", "uniform", "unwritten")


class QualityConfig(Struct):
    """fovpt_quality_config: which sums beside the per-class errors, and the width of a ring of the eccentricity profile
    (defaults: fovpt_quality_defaults)."""
    _fields_ = [("flags", C.c_int32), ("ring_width", C.c_int32), ("_reserved", C.c_int32 * 6)]


class QualitySums(Struct):
    """fovpt_quality_sums: the exact integer sums of one measurement, per class (QUALITY_FOVEA ..) and per ring."""
    _fields_ = [
        ("pixels", C.c_uint64 * 5), ("differing", C.c_uint64 * 5), ("sq_err", (C.c_uint64 * 3) * 5),
        ("max_err", C.c_uint32 * 5), ("_pad", C.c_uint32),
        ("windows", C.c_uint64 * 5), ("ssim_q20", C.c_int64 * 5),
        ("ring_pixels", C.c_uint64 * 64), ("ring_sq_err", C.c_uint64 * 64),
        ("width", C.c_uint32), ("height", C.c_uint32), ("ring_width", C.c_uint32), ("flags", C.c_uint32),
    ]

    def as_dict(self):
        """Every field: the arrays as (nested) lists of Python integers."""
        def val(v):
            return [val(x) for x in v] if isinstance(v, C.Array) else int(v)
        return {n: val(getattr(self, n)) for n, _ in self._fields_}


PACKET_MAGIC, PACKET_VERSION, PACKET_SLOTS =0x4b505646, 1, 4      # FOVPT_PACKET_*
PACKET_NEAREST, PACKET_SMOOTH = 0, 1
PACKET_MAGIC_CODED = 0x43505646                                   # "FVPC": a coded packet, a codec per pass
PACKET_RAW, PACKET_BC1, PACKET_BY_FILL = 0, 1, 0xffffffff


class PacketPass(Struct):
    """fovpt_packet_pass: a pass's launch grid, factor, fill and offset, and the byte offset of its texel array in the packet."""
    _fields_ = [
        ("gw", C.c_uint32), ("gh", C.c_uint32), ("factor", C.c_uint32), ("fill", C.c_uint32),
        ("offx", C.c_uint32), ("offy", C.c_uint32), ("texels", C.c_uint32), ("_reserved", C.c_uint32),
    ]


class PacketConfig(Struct):
    """fovpt_packet_config: the codec of every launch pass of a coded packet (PACKET_RAW, PACKET_BC1, PACKET_BY_FILL)."""
    _fields_ = [("codec", C.c_uint32 * 3), ("_reserved", C.c_uint32)]


class PacketHeader(Struct):
    """fovpt_packet_header: the first 128 bytes of a foveated frame packet, raw ("FVPK") or coded ("FVPC": a pass's _reserved is
    its codec)."""
    _fields_ = [
        ("magic", C.c_uint32), ("version", C.c_uint32), ("bytes", C.c_uint32), ("sequence", C.c_uint32),
        ("width", C.c_int32), ("height", C.c_int32), ("npass", C.c_uint32), ("_reserved", C.c_uint32),
        ("passes", PacketPass * 3),
    ]

    @classmethod
    def from_packet(cls, data):
        """The header of a packet's bytes (unchecked: fovpt_packet_check checks)."""
        return cls.from_buffer_copy(bytes(data[:C.sizeof(cls)]))


class Stats(Struct):
    _fields_ = [
        ("radiance_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("paths", C.c_uint64), ("frames", C.c_uint64),
        ("ms_generate", C.c_double), ("ms_trace", C.c_double), ("ms_shade", C.c_double),
        ("ms_shadow", C.c_double), ("ms_resolve", C.c_double),
        ("n_trace_launches", C.c_uint64), ("n_shadow_launches", C.c_uint64),
        ("num_triangles", C.c_uint64), ("num_bvh_nodes", C.c_uint64), ("bvh_max_depth", C.c_uint64),
        ("bvh_bytes", C.c_uint64), ("tri_bytes", C.c_uint64), ("ms_bvh_build", C.c_double),
    ]


class FramePtrs(Struct):
    _fields_ = [
        ("frame_buffer", C.c_void_p), ("accum_buffer", C.c_void_p), ("color_buffer", C.c_void_p),
        ("normal_buffer", C.c_void_p), ("albedo_buffer", C.c_void_p),
    ]


assert C.sizeof(Material) == 104
assert C.sizeof(Probe) == 64
assert C.sizeof(LaunchParams) == 248
assert C.sizeof(DenoiseConfig) == 32
assert C.sizeof(ReconstructConfig) == 32 and C.sizeof(GBufferPtrs) == 40
assert C.sizeof(TemporalConfig) == 32
assert C.sizeof(PostConfig) == 112 and (PostConfig.denoise.offset, PostConfig.reconstruct.offset, PostConfig.temporal.offset) == (16, 48, 80)
assert C.sizeof(ExposeConfig) == 80 and (ExposeConfig.low_permille.offset, ExposeConfig.key.offset) == (32, 48)
assert C.sizeof(ExposeState) == 32 and ExposeState.weight_total.offset == 16
assert C.sizeof(BloomConfig) == 64 and (BloomConfig.exposure.offset, BloomConfig.gain_fovea.offset, BloomConfig._reserved.offset) == (16, 28, 44)
assert C.sizeof(WarpCamera) == 48 and C.sizeof(WarpConfig) == 32 and C.sizeof(WarpCounts) == 32
assert C.sizeof(WarpMotionConfig) == 32 and WarpMotionConfig.advance.offset == 8
assert C.sizeof(FocusConfig) == 64 and (FocusConfig.strength.offset, FocusConfig._reserved.offset) == (16, 36)
assert C.sizeof(FocusState) == 32 and FocusState.count.offset == 16
assert C.sizeof(QualityConfig) == 32 and QualityConfig._reserved.offset == 8
assert C.sizeof(QualitySums) == 1344 and (QualitySums.max_err.offset, QualitySums.windows.offset, QualitySums.ring_pixels.offset, QualitySums.width.offset) == (200, 224, 304, 1328)
assert C.sizeof(LensConfig) == 128 and (LensConfig.k.offset, LensConfig.clip_r2.offset, LensConfig.border.offset, LensConfig._reserved.offset) == (32, 60, 80, 96)
assert C.sizeof(VarianceConfig) == 32 and (VarianceConfig.depth_tolerance.offset, VarianceConfig._reserved.offset) == (12, 20)
assert C.sizeof(VarianceFilterConfig) == 48 and (VarianceFilterConfig.luminance_sigma.offset, VarianceFilterConfig.demodulate.offset, VarianceFilterConfig._reserved.offset) == (16, 28, 32)
assert C.sizeof(PacketPass) == 32 and PacketPass.texels.offset == 24
assert C.sizeof(PacketConfig) == 16 and PacketConfig._reserved.offset == 12
assert C.sizeof(PacketHeader) == 128 and (PacketHeader.width.offset, PacketHeader.passes.offset) == (16, 32)
assert C.sizeof(VertexUpdate) == 16 and VertexUpdate.vertex.offset == 8
assert C.sizeof(MeshTransform) == 52 and MeshTransform.m.offset == 4
assert C.sizeof(HierarchyCost) == 32 and HierarchyCost.updates.offset == 16
assert C.sizeof(RebuildInfo) == 64 and (RebuildInfo.requested.offset, RebuildInfo.snapshot_update.offset, RebuildInfo.ms_build.offset) == (8, 48, 56)
assert C.sizeof(MeshSkin) == 32 and (MeshSkin.joints.offset, MeshSkin.weights.offset) == (16, 24)
assert C.sizeof(SkinPose) == 16 and SkinPose.matrices.offset == 8
assert C.sizeof(MorphTarget) == 24 and (MorphTarget.index.offset, MorphTarget.delta.offset) == (8, 16)
assert C.sizeof(MeshMorph) == 24 and MeshMorph.targets.offset == 16
assert C.sizeof(RigNode) == 44 and C.sizeof(RigBinding) == 32 and C.sizeof(RigChannel) == 32 and C.sizeof(RigClip) == 16 and C.sizeof(RigDesc) == 48
assert C.sizeof(MorphPose) == 32 and (MorphPose.weights.offset, MorphPose.num_joints.offset, MorphPose.matrices.offset) == (8, 16, 24)
assert LaunchParams.camera.offset == 104 and LaunchParams.traversable.offset == 160
assert LaunchParams.probe.offset == 168 and LaunchParams.viewportSize.offset == 232
assert _Frame.c.offset == 72 and _Frame.offset.offset == 88 and _Frame.size.offset == 40
