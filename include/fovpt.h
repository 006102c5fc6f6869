/*
 * fovpt.h -- C ABI of libfovpt, the MI355X (gfx950) foveated path-tracing launch.
 *
 * This is the drop-in boundary for ONE hot path of the reference renderer
 * (bipul-mohanto/fovPathTracing_optixCodeLatest): the per-frame foveated launch
 *   SampleRenderer::render()            PT_sv5_/SimplePathtracer.cpp:77-214
 *     -> 3 x optixLaunch                PT_sv5_/SimplePathtracer.cpp:148-209
 *       -> __raygen__renderFrame        PT_sv5_/deviceProgram.cu:392-617
 *       -> __closesthit__radiance       PT_sv5_/deviceProgram.cu:619-732
 *       -> miss / occlusion programs    PT_sv5_/deviceProgram.cu:253-300
 * Everything the reference obtained from OptiX for that path (accel build,
 * traversal, SBT, launch) lives behind these entry points.  Plain pointers and
 * sizes only; no C++ or torch types.  Every function returns 0 on success and
 * a negative FOVPT_E_* code on failure; fovpt_last_error() gives the text
 * (the reference throws sutil::Exception, sutil/Exception.h:93-193 -- the C++
 * shim in SimplePathtracer.h converts codes back into std::runtime_error).
 *
 * All structs below are bit-compatible with the reference's device-visible
 * structs as built by nvcc (8-byte aligned int2/uint2/float2, 16-byte float4):
 *   fovpt_material        == Material              PT_sv5_/Material.h:11-70      (104 B)
 *   fovpt_probe           == Probe                 PT_sv5_/Probe.cuh:6-21        ( 64 B)
 *   fovpt_launch_params   == LaunchParams          PT_sv5_/LaunchParams.h:49-91  (248 B)
 */
#ifndef FOVPT_H
#define FOVPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FOVPT_OK              0
#define FOVPT_E_INVALID      -1  /* bad argument / inconsistent sizes            */
#define FOVPT_E_DEVICE       -2  /* a HIP runtime call failed                     */
#define FOVPT_E_NO_SCENE     -3  /* launch before fovpt_set_scene                 */
#define FOVPT_E_NO_PROBE     -4  /* launch with a null probe                      */
#define FOVPT_E_NO_FRAME     -5  /* launch with null frame buffers                */
#define FOVPT_E_BVH_DEPTH    -6  /* built hierarchy deeper than the traversal stack */
#define FOVPT_E_NOMEM        -7

/* ---- POD vectors (layout of CUDA vector_types.h) --------------------------- */
typedef struct { float x, y, z; } fovpt_float3;
typedef struct { float x, y, z, w; } fovpt_float4;
typedef struct { int32_t x, y; } fovpt_int2;
typedef struct { uint32_t x, y; } fovpt_uint2;
typedef struct { uint32_t x, y, z; } fovpt_uint3;

/* ---- Material: PT_sv5_/Material.h:48-69 ------------------------------------ */
#define FOVPT_MATERIAL_FLAG_SHADOW_CATCHER 1 /* Material.h:9 */
typedef struct fovpt_material {
    fovpt_float3 emission;      /*   0 */
    fovpt_float3 color;         /*  12 */
    fovpt_float3 absorption;    /*  24 */
    float eta;                  /*  36 */
    float metallic;             /*  40 */
    float subsurface;           /*  44 */
    float specular;             /*  48 */
    float roughness;            /*  52 */
    float specularTint;         /*  56 */
    float anisotropic;          /*  60 */
    float sheen;                /*  64 */
    float sheenTint;            /*  68 */
    float clearcoat;            /*  72 */
    float clearcoatGloss;       /*  76 */
    float transmission;         /*  80 */
    float bump;                 /*  84 */
    fovpt_float3 bumpTile;      /*  88 */
    int32_t flags;              /* 100 */
} fovpt_material;               /* 104 */

/* ---- Probe: PT_sv5_/Probe.cuh:6-21 (device pointers) ----------------------- */
typedef struct fovpt_probe {
    int32_t width;              /*  0 */
    int32_t height;             /*  4 */
    fovpt_float4* data;         /*  8 */
    fovpt_float3 offset;        /* 16 */
    uint32_t _pad0;             /* 28 */
    float* pdfValuesX;          /* 32 */
    float* cdfValuesX;          /* 40 */
    float* pdfValuesY;          /* 48 */
    float* cdfValuesY;          /* 56 */
} fovpt_probe;                  /* 64 */

/* ---- LaunchParams: PT_sv5_/LaunchParams.h:49-91 ----------------------------- */
typedef struct fovpt_launch_params {
    struct {
        fovpt_float4* accum_buffer;  /*   0  float4 per pixel, device            */
        uint32_t* frame_buffer;      /*   8  rgba8 per pixel (uchar4), device    */
        fovpt_float4* color_buffer;  /*  16  dead in sv5                         */
        fovpt_float4* normal_buffer; /*  24  dead in sv5                         */
        fovpt_float4* albedo_buffer; /*  32  dead in sv5                         */
        fovpt_int2 size;             /*  40                                      */
        uint32_t subframe_index;     /*  48                                      */
        fovpt_uint3 factor;          /*  52                                      */
        int32_t fillSize;            /*  64                                      */
        uint32_t _pad0;              /*  68                                      */
        fovpt_uint2 c;               /*  72  gaze centre, pixels                 */
        float r_inner;               /*  80                                      */
        float r_outer;               /*  84                                      */
        fovpt_uint2 offset;          /*  88                                      */
        uint32_t redraw;             /*  96                                      */
        uint32_t _pad1;              /* 100                                      */
    } frame;
    struct {
        fovpt_float3 eye;            /* 104 */
        fovpt_float3 U;              /* 116 */
        fovpt_float3 V;              /* 128 */
        fovpt_float3 W;              /* 140 */
    } camera;
    uint32_t samples_per_launch;     /* 152 */
    uint32_t _pad2;                  /* 156 */
    uint64_t traversable;            /* 160  scene handle from fovpt_set_scene   */
    fovpt_probe probe;               /* 168 */
    fovpt_int2 viewportSize;         /* 232  dead in sv5                         */
    float white;                     /* 240  dead in sv5                         */
    uint32_t _pad3;                  /* 244 */
} fovpt_launch_params;               /* 248 */

/* ---- scene upload: replaces buildAccel + createTextures + buildSBT ----------
 * (PT_sv5_/SimplePathtracer.cpp:602-746, 748-799, 534-599).  Host pointers;
 * everything is copied before the call returns.                                */
typedef struct fovpt_mesh_desc {
    const float* vertex;        /* xyz triples, TriangleMesh::vertex  (Model.h:12) */
    const float* normal;        /* xyz triples or NULL; the path never reads them
                                   (deviceProgram.cu:632-634 uses the face normal) */
    const float* texcoord;      /* uv pairs per vertex or NULL        (Model.h:14) */
    const uint32_t* index;      /* 3 per triangle                     (Model.h:15) */
    uint32_t num_vertices;
    uint32_t num_triangles;
    int32_t texture_id;         /* TriangleMesh::diffuseTextureID; <0 = untextured */
    fovpt_material material;
} fovpt_mesh_desc;

typedef struct fovpt_texture_desc {
    const uint32_t* pixel;      /* RGBA8, row-major, Texture::pixel (Model.h:27)   */
    int32_t width, height;      /* Texture::resolution                             */
} fovpt_texture_desc;

/* ---- run-time configuration (the reference's compile-time #defines) ---------
 * Defaults reproduce PT_sv5_ as shipped: FOV_ON, radii 74/241
 * (SimplePathtracer.cpp:20-23), spp 8/16/32 (:142,170,193), uniform spp 4 (:95),
 * depth cap 4 (deviceProgram.cu:515), accumulate off (:565-581).               */
typedef struct fovpt_config {
    int32_t uniform;            /* 1 = FOV_OFF branch (SimplePathtracer.cpp:85-131) */
    int32_t r_inner;            /* inner_radius                                    */
    int32_t r_outer;            /* outer_radius                                    */
    int32_t spp_periphery;      /* samples_per_launch of pass P                    */
    int32_t spp_middle;         /* ... pass M                                      */
    int32_t spp_fovea;          /* ... pass F                                      */
    int32_t spp_uniform;        /* ... FOV_OFF                                     */
    int32_t max_depth;          /* depth cap, deviceProgram.cu:515                 */
    int32_t accumulate;         /* 1 = PT_sv4_vmv2 clamp(0,10)+running mean
                                   (OtherProjects_02_latest/PT_sv4_vmv2/deviceProgram.cu:545-553) */
    int32_t rank;               /* multi-GPU tile shard: this handle renders the   */
    int32_t world;              /* launch-index tiles t with owner(t) == rank      */
    int32_t tile_w, tile_h;     /* launch-index tile, default 8 x 4
                                   (sutil/WorkDistribution.h:47-84 scheme)         */
    int32_t profile;            /* 1 = time each kernel with hipEvents; 2 = the same with every kernel
                                   run ALONE (host synchronisation around it: serialised times)     */
    int32_t write_guides;       /* 1 = also write normal/color/albedo_buffer, the denoiser guides of
                                   PT_sv/deviceProgram.cu:555-557 (commented out in PT_sv5_, :612-614);
                                   not available with shadow-catcher materials         */
    int32_t options;            /* opt-in extensions beyond the reference's behaviour (0 = PT_sv5_ as shipped):
                                   FOVPT_OPT_SKY_MISS, FOVPT_OPT_RUSSIAN_ROULETTE                     */
    int32_t frames_in_flight;   /* jobs (frames issued without fovpt_synchronize between them) whose main chains --
                                   generate, closest hit, shade, one after the other -- may run BESIDE each other:
                                   0 = the library's default (2), 1 = one frame at a time (lowest latency per frame),
                                   2 = two (highest throughput: each chain fills the other's gaps; a frame then takes
                                   about twice as long from first to last kernel); 3 and 4 are accepted and measured slower
                                   than 2 (a context has FOVPT_LANES = 2 stream pairs unless the environment says more; a
                                   larger value means all of them).  Results do not depend on it: resolves
                                   run in issue order, and fovpt_stream() is ordered behind every finished frame.
                                   (Path state and queues exist once per state set; jobs of up to 16 Mi sample slots rotate
                                   through twice as many sets as stream pairs -- FOVPT_SETS -- so that a frame's head does
                                   not wait for the resolve of the frame two before it.)                                 */
    int32_t chains_per_frame;   /* 0 / 1 = a frame is one chain of dependent launches; 2 = every frame is rendered as TWO
                                   independent chains over halves of its sample slots (each with four of the eight queue
                                   shards, on its own stream pair) and resolved once: frames issued back to back then
                                   follow each other as closely as with frames_in_flight = 2 while each is finished in
                                   about half the time after its issue (one frame in flight instead of two).  It does not
                                   shorten a frame for a caller that synchronises after every frame (measured), and costs
                                   2-5 % of the throughput on multi-million-triangle scenes.  With 2, frames are issued one
                                   at a time (frames_in_flight is ignored).  Results do not depend on it.              */
} fovpt_config;

/* fovpt_config.options.  Both are NON-PARITY modes with respect to the reference (it has neither); the CPU oracle
 * implements them identically, so the GPU is still checked bit for bit against it.
 *  SKY_MISS          the multiple-importance-sampling counterpart of SampleLights that PT_sv5_ carries commented out
 *                    in __miss__radiance (deviceProgram.cu:259-269, :273-278): a SECONDARY ray that escapes adds
 *                    w * ProbeEval(dir) * pathThroughput, w = bsdfPdf / (bsdfPdf + ProbePdf(dir)) (Probe.cuh:69-93), and the
 *                    path loop counts that segment although it is DONE (the reference's break at :515 would drop it).
 *  RUSSIAN_ROULETTE  the //!TODO of deviceProgram.cu:518-520: from the second bounce on a path survives a shaded hit
 *                    with probability q = clamp(max component of pathThroughput, 0.05, 1), decided by one more
 *                    Random::Randf() after BSDFSample's draws; survivors carry pathThroughput / q.                */
#define FOVPT_OPT_SKY_MISS 1
#define FOVPT_OPT_RUSSIAN_ROULETTE 2

typedef struct fovpt_stats {
    uint64_t radiance_rays;     /* closest-hit rays traced since last reset        */
    uint64_t shadow_rays;       /* occlusion rays traced                           */
    uint64_t paths;             /* camera paths started                            */
    uint64_t frames;            /* fovpt_render / fovpt_launch calls               */
    /* per-kernel device time, only filled when config.profile = 1 or 2           */
    double ms_generate, ms_trace, ms_shade, ms_shadow, ms_resolve;
    uint64_t n_trace_launches;  /* closest-hit kernel launches behind ms_trace     */
    uint64_t n_shadow_launches;
    /* scene facts */
    uint64_t num_triangles, num_bvh_nodes, bvh_max_depth, bvh_bytes, tri_bytes;
    double ms_bvh_build;
} fovpt_stats;

typedef struct fovpt_frame_ptrs {   /* what resize() allocates, SimplePathtracer.cpp:242-260 */
    uint32_t* frame_buffer;
    fovpt_float4* accum_buffer;
    fovpt_float4* color_buffer;
    fovpt_float4* normal_buffer;
    fovpt_float4* albedo_buffer;
} fovpt_frame_ptrs;

typedef struct fovpt_ctx fovpt_ctx;

/* SampleRenderer ctor minus the scene: initOptix/createContext (SimplePathtracer.cpp:310-340). */
int fovpt_create(fovpt_ctx** out, int device);
void fovpt_destroy(fovpt_ctx* ctx);
const char* fovpt_last_error(const fovpt_ctx* ctx);  /* ctx may be NULL: last create error */

/* buildAccel + createTextures + buildSBT.  *traversable_out is what the reference
 * stores in launchParams.traversable (SimplePathtracer.cpp:61).  At most 2^26
 * triangles in total (FOVPT_E_INVALID beyond: the traversal addresses the 48-byte
 * triangle records and 128-byte nodes with 32-bit byte offsets); a hierarchy deeper
 * than 21 four-wide levels is refused with FOVPT_E_BVH_DEPTH.                      */
int fovpt_set_scene(fovpt_ctx* ctx, const fovpt_mesh_desc* meshes, int num_meshes,
                    const fovpt_texture_desc* textures, int num_textures,
                    uint64_t* traversable_out);

/* ---- animated geometry: new vertex positions for meshes of the current scene ---------------------------------------------
 * New with this library: the reference builds its acceleration structure once (SimplePathtracer.cpp:671-706, no ALLOW_UPDATE);
 * this is the counterpart of optixAccelBuild with OPERATION_UPDATE over the same build inputs.
 *   geometry   the named meshes get new positions, every other mesh keeps the positions it last had.  Indices, texcoords,
 *              materials, textures, primitive ids, the traversable handle and the temporal history stay as they are.  After
 *              the call every frame, G-buffer and fovpt_debug_trace is bit for bit what a context gets from fovpt_set_scene with
 *              the updated meshes (a hit is the minimum (t, primitive id), occlusion is existence: neither depends on the tree).
 *   refit      (the default) keeps the tree and recomputes, deepest level first, every leaf's triangle records and the boxes
 *              of the hierarchy (the same padded triangle boxes the build unions).  Asynchronous and stream-ordered, no host
 *              synchronisation: it runs after every frame, job, G-buffer and debug trace issued before the call, whatever
 *              frames_in_flight and chains_per_frame say, and everything issued after the call sees the new geometry.  Host
 *              vertex data is copied before the call returns (through a pinned staging buffer, as fovpt_set_scene copies).
 *              With FOVPT_UPDATE_DEVICE the vertex pointers are device pointers, read in stream order on fovpt_stream(): the
 *              caller orders its own writes of them before the call.  A refit tree keeps its shape: traversal slows as the
 *              motion grows, which FOVPT_UPDATE_REBUILD resets.
 *   REBUILD    builds the hierarchy anew over the updated (current) vertices, as fovpt_set_scene builds it.  Host-synchronous
 *              like fovpt_set_scene; keeps the handle, primitive ids and history.  Updates stats.ms_bvh_build and the scene facts
 *              as fovpt_set_scene does (a refit leaves them unchanged).  num_updates may be 0: a rebuild alone.  If the build
 *              fails (FOVPT_E_BVH_DEPTH, FOVPT_E_DEVICE) the previous hierarchy stays.
 *   errors     all or nothing, checked before anything changes.  FOVPT_E_NO_SCENE: no scene.  FOVPT_E_INVALID: null ctx, null
 *              updates with num_updates > 0, num_updates < 0, a mesh out of range or listed twice, num_vertices other than the
 *              mesh's, a null vertex pointer, unknown flag bits, a non-finite coordinate (host data only: device data is not
 *              read by the call, and non-finite device coordinates are the caller's responsibility).
 *              num_updates == 0 without FOVPT_UPDATE_REBUILD: FOVPT_OK, nothing happens.
 * Device memory: on the first update the context keeps the vertex positions (12 bytes per vertex) and the vertex indices of
 * every triangle (12 bytes per triangle); a scene that is never updated costs nothing more on the device.                 */
typedef struct fovpt_vertex_update {
    int32_t mesh;                /* index into the meshes given to fovpt_set_scene                                          */
    uint32_t num_vertices;       /* must equal that mesh's num_vertices                                                     */
    const float* vertex;         /* xyz triples (host, or device with FOVPT_UPDATE_DEVICE)                                  */
} fovpt_vertex_update;
#define FOVPT_UPDATE_DEVICE  1   /* vertex pointers are device pointers, read in stream order on fovpt_stream()             */
#define FOVPT_UPDATE_REBUILD 2   /* build the hierarchy anew over the updated vertices instead of refitting it              */
int fovpt_update_vertices(fovpt_ctx* ctx, const fovpt_vertex_update* updates, int num_updates, int flags);

/* ---- rigid (affine) motion: per-mesh transforms applied on the device ------------------------------------------------------
 * fovpt_update_vertices for meshes that only turn, travel, scale or shear: twelve numbers per mesh instead of its vertices.
 *   geometry   every vertex (x, y, z) of a named mesh's REST positions -- the ones fovpt_set_scene received, not the mesh's
 *              current ones -- becomes
 *                  x' = ((m[0] * x + m[1] * y) + m[2] * z) + m[3]        y', z': the same with rows 1 and 2
 *              every * and + one unfused binary32 operation.  Transforms are absolute: M1 then M2 leaves M2 . rest, and a mesh
 *              fovpt_update_vertices has deformed is set from rest again.  Meshes not named keep what they last had, through
 *              either call.  (An identity matrix turns a coordinate of -0 into +0: -0 + +0 = +0.)
 *   contract   after the call every frame, G-buffer, debug trace, "scene_vertices" buffer and hierarchy byte is what
 *              fovpt_update_vertices gives on the same context with those x', y', z' as host arrays.  Stream ordering, the
 *              refit, fovpt_temporal_motion's tracking and FOVPT_UPDATE_REBUILD (the only flag accepted) are that call's own.
 *   errors     all or nothing, checked before anything changes.  FOVPT_E_NO_SCENE: no scene.  FOVPT_E_INVALID: null ctx, null
 *              transforms with num > 0, num < 0, a mesh out of range or listed twice, flag bits other than
 *              FOVPT_UPDATE_REBUILD, a non-finite matrix entry, or a matrix that could overflow: with A the largest
 *              |coordinate| of the mesh's rest positions, a row with (|m0| + |m1| + |m2|) * A + |m3| > 2^127 (in binary64).
 *              Below that bound every intermediate value is finite.  Singular matrices are allowed.
 *              num == 0 without FOVPT_UPDATE_REBUILD: FOVPT_OK, nothing happens.
 * Device memory: the first call keeps a device copy of the rest positions (12 bytes per vertex) until the next
 * fovpt_set_scene; a context that never calls it pays nothing.                                                              */
typedef struct fovpt_mesh_transform {
    int32_t mesh;                /* index into the meshes given to fovpt_set_scene                                          */
    float m[12];                 /* row-major 3 x 4: row r is m[4r .. 4r+3]                                                 */
} fovpt_mesh_transform;
int fovpt_update_transforms(fovpt_ctx* ctx, const fovpt_mesh_transform* transforms, int num, int flags);

/* ---- skinning: per-mesh joint palettes blended on the device -----------------------------------------------------------------
 * fovpt_update_vertices for skinned meshes (linear-blend skinning, four influences): the skin is uploaded once per mesh with
 * fovpt_set_skins, and every frame carries a palette of joint matrices, 48 bytes per joint instead of 12 bytes per vertex.
 *   geometry   for a vertex of a named mesh with REST position (x, y, z) -- the one fovpt_set_scene received --, joints
 *              j0 .. j3, weights w0 .. w3 and the palette J of row-major 3 x 4 matrices, each entry e = 0 .. 11 of the blended
 *              matrix is
 *                  M[e] = ((w0 * J[j0][e] + w1 * J[j1][e]) + w2 * J[j2][e]) + w3 * J[j3][e]
 *              and
 *                  x' = ((M[0] * x + M[1] * y) + M[2] * z) + M[3]        y', z': the same with rows 1 and 2
 *              every * and + one unfused binary32 operation.  Weights are used as given, NOT normalised.  Poses are absolute:
 *              P1 then P2 leaves P2 applied to rest, and a mesh fovpt_update_vertices or fovpt_update_transforms has moved is
 *              set from rest again.  Meshes not named keep what they last had, through any of the three calls; a skinned mesh
 *              may still be given to the other two.
 *   contract   after the call every frame, G-buffer, debug trace, "scene_vertices" buffer and hierarchy byte is what
 *              fovpt_update_vertices gives on the same context with those x', y', z' as host arrays.  Stream ordering, the
 *              refit, fovpt_temporal_motion's tracking, fovpt_hierarchy_cost's counting and FOVPT_UPDATE_REBUILD are that call's
 *              own.
 *   set_skins  set-up-time state of the scene: each entry sets, replaces or (num_joints == 0, both pointers null) removes the
 *              skin of its mesh; the skins of other meshes stay; fovpt_set_scene drops them all.  Everything is copied before
 *              the call returns; it may synchronise fovpt_stream(); it does not move geometry.  Per mesh the library keeps S,
 *              the largest w0 + w1 + w2 + w3 over the mesh's vertices (in binary64), for the overflow rule below.
 *              All or nothing.  FOVPT_E_NO_SCENE: no scene.  FOVPT_E_INVALID: null ctx, null skins with num > 0, num < 0, a
 *              mesh out of range or listed twice, num_vertices other than the mesh's, num_joints above FOVPT_SKIN_MAX_JOINTS,
 *              one null pointer of the pair (or both with num_joints > 0), non-zero _reserved, a joint index >= num_joints
 *              (also where its weight is 0), a weight that is NaN, infinite, negative or above 1.
 *   poses      fovpt_update_skinned: matrices are host memory, copied before the call returns (through a pinned staging
 *              buffer into a palette the context owns), or with FOVPT_UPDATE_DEVICE device memory read in place in stream
 *              order on fovpt_stream() and not validated, as fovpt_update_vertices' device pointers are.
 *              All or nothing, checked before anything changes.  FOVPT_E_NO_SCENE: no scene.  FOVPT_E_INVALID: null ctx, null
 *              poses with num > 0, num < 0, a mesh out of range or listed twice, a mesh without a skin, num_joints other than
 *              the skin's, a null matrices pointer, unknown flag bits, and for host matrices a non-finite entry or a matrix that
 *              could overflow: with A the largest |coordinate| of the mesh's rest positions and S as above, a row with
 *              S * ((|m0| + |m1| + |m2|) * A + |m3|) > 2^127 (in binary64), or an entry with S * |m| > 2^127.  With S = 1
 *              the first is fovpt_update_transforms' rule: every partial sum of a blended row applied to a vertex is bounded
 *              by that expression.  The second bounds the entries of M themselves, which the first does only when A >= 1.
 *              Within both every intermediate value is finite.  num == 0 without FOVPT_UPDATE_REBUILD: FOVPT_OK, nothing
 *              happens.
 * Memory: 24 bytes per skinned vertex on the device (8 of joint indices, 16 of weights) and the same on the host, 48 bytes per
 * joint of palette, and the device copy of the rest positions fovpt_update_transforms makes (12 bytes per vertex, one copy shared
 * by both, made on the first call of either).  A context that never calls these functions pays nothing.                      */
#define FOVPT_SKIN_MAX_JOINTS 1024
typedef struct fovpt_mesh_skin {
    int32_t mesh;                /* index into the meshes given to fovpt_set_scene                                          */
    uint32_t num_vertices;       /* must equal that mesh's num_vertices                                                     */
    uint32_t num_joints;         /* 1 .. FOVPT_SKIN_MAX_JOINTS; 0 with joints == weights == NULL: remove                    */
    uint32_t _reserved;          /* 0                                                                                       */
    const uint16_t* joints;      /* 4 per vertex, host, every one < num_joints (also where its weight is 0)                 */
    const float* weights;        /* 4 per vertex, host, each finite and 0 <= w <= 1; NOT normalised by the library          */
} fovpt_mesh_skin;               /* 32 bytes */
int fovpt_set_skins(fovpt_ctx* ctx, const fovpt_mesh_skin* skins, int num);

typedef struct fovpt_skin_pose {
    int32_t mesh;                /* index into the meshes given to fovpt_set_scene                                          */
    uint32_t num_joints;         /* must equal the mesh's skin's                                                            */
    const float* matrices;       /* num_joints row-major 3 x 4 matrices, 12 floats each (host, or device with FOVPT_UPDATE_DEVICE) */
} fovpt_skin_pose;               /* 16 bytes */
int fovpt_update_skinned(fovpt_ctx* ctx, const fovpt_skin_pose* poses, int num, int flags);   /* FOVPT_UPDATE_DEVICE | FOVPT_UPDATE_REBUILD */

/* ---- morph targets: per-mesh blend shapes weighted on the device --------------------------------------------------------------
 * fovpt_update_vertices for morphed meshes (blend shapes: a face, a muscle corrective, cloth keyframes): the targets are
 * uploaded once per mesh with fovpt_set_morphs, and every frame carries one weight per target, a few hundred bytes instead of
 * 12 bytes per vertex.  With a palette the morphed positions go through the mesh's skin in the same pass (glTF's order: morph,
 * then skin).
 *   geometry   for a vertex of a named mesh with REST position p = (x, y, z) -- the one fovpt_set_scene received --, the mesh's
 *              targets t = 0, 1, ... in ascending order: for every target that lists the vertex, with delta d, and whose weight
 *              has w[t] != 0.0f,
 *                  p.x = p.x + w[t] * d.x        p.y, p.z likewise
 *              every * and + one unfused binary32 operation.  A target whose weight is +0 or -0 is SKIPPED, not applied: a pose
 *              of all zeros leaves rest bit for bit, a coordinate of -0 included.  Zero deltas are applied like any other entry;
 *              weights may be negative or above 1.  With matrices the morphed p then goes through fovpt_update_skinned's
 *              expression unchanged, with the mesh's skin from fovpt_set_skins: the blended M[e], then
 *              x' = ((M[0] * x + M[1] * y) + M[2] * z) + M[3].  Poses are absolute and start from rest; meshes not named keep
 *              what they last had, through any of the four calls; a morphed mesh may still be given to the other three, and
 *              fovpt_update_skinned of a morphed mesh is rest through the skin.
 *   contract   after the call every frame, G-buffer, debug trace, "scene_vertices" buffer and hierarchy byte is what
 *              fovpt_update_vertices gives on the same context with those positions as host arrays.  Stream ordering, the
 *              refit, fovpt_temporal_motion's tracking, fovpt_hierarchy_cost's counting and FOVPT_UPDATE_REBUILD are that call's
 *              own.
 *   set_morphs set-up-time state of the scene: each entry sets, replaces or (num_targets == 0, targets null) removes the morphs
 *              of its mesh; the morphs of other meshes stay; fovpt_set_scene drops them all.  Everything is copied before the
 *              call returns; it may synchronise fovpt_stream(); it does not move geometry.  Per target the library keeps D_t,
 *              the largest |delta component| (in binary64; 0 for an empty target), for the overflow rule below.
 *              All or nothing.  FOVPT_E_NO_SCENE: no scene.  FOVPT_E_INVALID: null ctx, null morphs with num > 0, num < 0, a
 *              mesh out of range or listed twice, num_vertices other than the mesh's, num_targets above
 *              FOVPT_MORPH_MAX_TARGETS, targets null with num_targets > 0 or non-null with num_targets == 0, a non-zero
 *              _reserved of either struct, count > num_vertices, a null index with 0 < count < num_vertices, a null delta with
 *              count > 0, indices not strictly ascending or >= num_vertices, a non-finite delta, more than 2^32 - 1 entries
 *              (index, delta pairs) in the scene's morphs together.
 *   poses      fovpt_update_morphed: weights and matrices are host memory, copied before the call returns (through a pinned
 *              staging buffer into arrays the context owns), or with FOVPT_UPDATE_DEVICE both are device memory read in place
 *              in stream order on fovpt_stream() and not validated.
 *              All or nothing, checked before anything changes.  FOVPT_E_NO_SCENE: no scene.  FOVPT_E_INVALID: null ctx, null
 *              poses with num > 0, num < 0, a mesh out of range or listed twice, a mesh without morphs, num_targets other than
 *              the mesh's, null weights, unknown flag bits, non-zero _reserved, matrices or num_joints on a mesh without a skin
 *              or with a num_joints other than the skin's, exactly one of matrices == NULL and num_joints == 0, and for host
 *              data a non-finite weight or matrix entry or a pose that could overflow: with A the largest |coordinate| of the
 *              mesh's rest positions,
 *                  B = A + sum over ascending t of |w[t]| * D_t        (in binary64)
 *              must not exceed 2^127; every partial sum of a morphed coordinate and every product w * d is within B.  With
 *              matrices, fovpt_update_skinned's two rules hold with B in A's place: no row with
 *              S * ((|m0| + |m1| + |m2|) * B + |m3|) > 2^127 and no entry of the first three columns with S * |m| > 2^127.
 *              Within the rules every intermediate value is finite.  num == 0 without FOVPT_UPDATE_REBUILD: FOVPT_OK, nothing
 *              happens.
 * Memory: 16 bytes per (vertex, target) entry and 4 bytes per vertex of a morphed mesh (+ 4 per mesh) on the device and the same
 * on the host, 4 bytes per target of weights, and the device copy of the rest positions shared with fovpt_update_transforms
 * and fovpt_update_skinned (12 bytes per vertex, made on the first call of any of the three).  A context that never calls these
 * functions pays nothing.                                                                                                     */
#define FOVPT_MORPH_MAX_TARGETS 256
typedef struct fovpt_morph_target {
    uint32_t count;              /* vertices this target moves, 0 .. num_vertices                                           */
    uint32_t _reserved;          /* 0                                                                                       */
    const uint32_t* index;       /* count vertex indices, host, strictly ascending, each < num_vertices; NULL = dense:
                                    count == num_vertices (or 0), entry i is vertex i                                       */
    const float* delta;          /* count xyz triples, host, finite; NULL only with count == 0                              */
} fovpt_morph_target;            /* 24 bytes */
typedef struct fovpt_mesh_morph {
    int32_t mesh;                /* index into the meshes given to fovpt_set_scene                                          */
    uint32_t num_vertices;       /* must equal that mesh's num_vertices                                                     */
    uint32_t num_targets;        /* 1 .. FOVPT_MORPH_MAX_TARGETS; 0 with targets == NULL: remove                            */
    uint32_t _reserved;          /* 0                                                                                       */
    const fovpt_morph_target* targets;   /* num_targets of them                                                             */
} fovpt_mesh_morph;              /* 24 bytes */
int fovpt_set_morphs(fovpt_ctx* ctx, const fovpt_mesh_morph* morphs, int num);

typedef struct fovpt_morph_pose {
    int32_t mesh;                /* index into the meshes given to fovpt_set_scene                                          */
    uint32_t num_targets;        /* must equal the mesh's                                                                   */
    const float* weights;        /* num_targets floats (host, or device with FOVPT_UPDATE_DEVICE)                           */
    uint32_t num_joints;         /* 0: morph alone; else must equal the mesh's skin's                                       */
    uint32_t _reserved;          /* 0                                                                                       */
    const float* matrices;       /* NULL with num_joints 0; else the mesh's skin palette, as fovpt_skin_pose.matrices       */
} fovpt_morph_pose;              /* 32 bytes */
int fovpt_update_morphed(fovpt_ctx* ctx, const fovpt_morph_pose* poses, int num, int flags);   /* FOVPT_UPDATE_DEVICE | FOVPT_UPDATE_REBUILD */

/* ---- rigs: keyframe clips sampled and composed on the device ------------------------------------------------------------------
 * fovpt_update_skinned / fovpt_update_morphed / fovpt_update_transforms without the caller's animation system: the node hierarchy,
 * the bindings of meshes to it and the keyframe clips are uploaded once with fovpt_set_rig, and every frame carries one number,
 * the time.  The layout maps onto glTF's nodes, skins and animation samplers one to one.
 *   sample     a channel with keys t_0 < ... < t_{n-1} at time T: T <= t_0 gives v_0, T >= t_{n-1} gives v_{n-1}; otherwise
 *              k is the largest index with t_k <= T.  FOVPT_RIG_STEP gives v_k.  FOVPT_RIG_LINEAR: u = (T - t_k) / (t_{k+1} - t_k)
 *              and, for translation, scale and weights, v = v_k + u * (v_{k+1} - v_k) per component (at a key, u = 0: the key,
 *              a component of -0 becoming +0).  For rotation, with a = v_k, b = v_{k+1}:
 *                  d = ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w;   if d < 0: b = -b, d = -d
 *                  d > 0.9995f:  q = a + u * (b - a)                                              per component
 *                  otherwise:    th = fovpt_dm_acosf(d), s = fovpt_dm_sinf(th), wa = fovpt_dm_sinf((1.0f - u) * th) / s,
 *                                wb = fovpt_dm_sinf(u * th) / s, q = wa * a + wb * b              per component
 *                  then q = q / sqrtf(((x * x + y * y) + z * z) + w * w)                          per component
 *              (include/fovpt_detmath.h: host and device agree bit for bit).  Every *, +, -, / and square root is one unfused
 *              binary32 operation.  Values that were not interpolated -- rest values, STEP, either end of a clip -- are used as
 *              given, NOT normalised (glTF's rule).  A path no channel of the clip names takes the node's rest value; a bound
 *              morphed mesh without a WEIGHTS channel in the clip gets all-zero weights (rest, through the skin where skinned).
 *   local      from (t, q = (x, y, z, w), s):  r00 = 1.0f - 2.0f * (y * y + z * z)   r01 = 2.0f * (x * y - z * w)   r02 = 2.0f * (x * z + y * w)
 *                                              r10 = 2.0f * (x * y + z * w)   r11 = 1.0f - 2.0f * (x * x + z * z)   r12 = 2.0f * (y * z - x * w)
 *                                              r20 = 2.0f * (x * z - y * w)   r21 = 2.0f * (y * z + x * w)   r22 = 1.0f - 2.0f * (x * x + y * y)
 *              L[r][c] = r_rc * s[c], L[r][3] = t[r].
 *   world      W = L for a root, otherwise W = P o L, P the parent's world:
 *                  (P o L)[r][c] = (P[r][0] * L[0][c] + P[r][1] * L[1][c]) + P[r][2] * L[2][c]                   c < 3
 *                  (P o L)[r][3] = ((P[r][0] * L[0][3] + P[r][1] * L[1][3]) + P[r][2] * L[2][3]) + P[r][3]
 *   palette    J[j] = W[joint_nodes[j]] o inverse_bind[j], the same product; a rigid binding's matrix is M = W[node].
 *   apply      a binding with joints goes through fovpt_update_skinned's expression with J (through fovpt_update_morphed's with the
 *              sampled weights and J where the mesh has morphs), a binding without joints on a morphed mesh through
 *              fovpt_update_morphed's with the weights alone, a rigid one through fovpt_update_transforms' with M.
 *   contract   after fovpt_update_animated every frame, G-buffer, debug trace, "scene_vertices" buffer and hierarchy byte is what
 *              fovpt_update_vertices gives on the same context with those positions of all bound meshes as host arrays in one
 *              call.  It is one update: stream ordering, the refit, fovpt_temporal_motion's tracking, fovpt_hierarchy_cost's
 *              counting (+1) and FOVPT_UPDATE_REBUILD (the only flag) are that call's own.  Meshes that are not bound keep what
 *              they last had; poses are absolute and start from rest; a bound mesh may still be given to the other four calls.
 *              Nothing but the kernel arguments crosses the bus.  The composed matrices are computed on the device and NOT
 *              validated (the rule for FOVPT_UPDATE_DEVICE pointers): overflow along a hierarchy is the caller's responsibility.
 *   set_rig    set-up-time state of the scene, called after fovpt_set_skins / fovpt_set_morphs: everything is validated first and
 *              copied before the call returns; it may synchronise fovpt_stream(); it does not move geometry; it replaces a
 *              previous rig as a whole (NULL: removes it).  A later fovpt_set_skins, fovpt_set_morphs or fovpt_set_scene drops
 *              the rig: its joint and target counts were checked against those.  All or nothing.  FOVPT_E_NO_SCENE: no scene.
 *              FOVPT_E_INVALID: null ctx; counts above the limits; num_nodes 0; a null array with a count > 0; a non-zero
 *              reserved field; a parent >= the node's own index or < -1; a non-finite rest value; a rest rotation whose squared
 *              norm (binary64) is outside [1/4, 4]; a binding's mesh out of range or bound twice; both node >= 0 and
 *              num_joints > 0; a node (< -1 or >= num_nodes) or joint node out of range; num_joints > 0 other than the mesh's
 *              skin's, or on a mesh without a skin; a rigid binding on a mesh that has morphs; a binding with neither node,
 *              joints nor morphs on its mesh; a null joint_nodes or inverse_bind with num_joints > 0; a non-finite inverse bind
 *              entry; a channel with an unknown path or interpolation, a target out of range, WEIGHTS on a mesh that is not
 *              bound or has no morphs, the same (target, path) twice in one clip, num_keys outside 1 .. FOVPT_RIG_MAX_KEYS,
 *              null times or values, times not finite or not strictly ascending, a non-finite value, a rotation key whose
 *              squared norm is outside [1/4, 4]; more than 2^32 - 1 key times or values in the rig together.
 *   animated   fovpt_update_animated poses every bound mesh from clip `clip` at `time`.  All or nothing.  FOVPT_E_NO_SCENE: no
 *              scene.  FOVPT_E_INVALID: null ctx, no rig, clip out of range, a non-finite time, flag bits other than
 *              FOVPT_UPDATE_REBUILD.  A rig without bindings: FOVPT_OK, nothing happens (unless a rebuild is asked for).
 * Memory: on the device 44 + 12 bytes per node and clip-table entries of 12 bytes per node and clip, 4 bytes per key time and per
 * key value, 56 bytes per joint of a binding, and 48 bytes per node, joint and rigid binding of results; nothing on the host
 * beyond the list of bindings.  One k_rig_pose launch (one workgroup, a thread per node, a barrier per level of the hierarchy)
 * ahead of the skinning, morph and transform launches: DESIGN.md, section 24.  Measured there on an MI355X, 103 meshes of 139 594
 * vertices bound over 3020 joints to a rig of 1024 nodes in 8 levels: 0.144 ms per fovpt_update_animated against 0.220 ms per
 * fovpt_update_skinned with host palettes made beforehand; k_rig_pose alone 0.004 ms for 1024 nodes on one level and 0.285 ms for
 * 1024 nodes in one chain (about 0.28 us per level).  A context that never calls these functions pays nothing.                */
#define FOVPT_RIG_MAX_NODES 1024
#define FOVPT_RIG_MAX_CLIPS 64
#define FOVPT_RIG_MAX_KEYS  (1u << 20)      /* per channel */
#define FOVPT_RIG_TRANSLATION 0
#define FOVPT_RIG_ROTATION    1
#define FOVPT_RIG_SCALE       2
#define FOVPT_RIG_WEIGHTS     3
#define FOVPT_RIG_STEP   0
#define FOVPT_RIG_LINEAR 1
typedef struct fovpt_rig_node {
    int32_t parent;              /* -1: a root; otherwise < this node's own index                                           */
    float translation[3], rotation[4] /* x y z w */, scale[3];   /* the rest pose                                          */
} fovpt_rig_node;                /* 44 bytes */
typedef struct fovpt_rig_binding {   /* one mesh the rig drives */
    int32_t mesh;                /* index into the meshes given to fovpt_set_scene                                          */
    int32_t node;                /* >= 0: the mesh follows this node rigidly (num_joints 0); -1 otherwise                   */
    uint32_t num_joints;         /* > 0: must equal the mesh's skin's (fovpt_set_skins)                                     */
    uint32_t _reserved;          /* 0                                                                                       */
    const uint16_t* joint_nodes; /* num_joints node indices, host                                                           */
    const float* inverse_bind;   /* num_joints row-major 3 x 4 matrices, host                                               */
} fovpt_rig_binding;             /* 32 bytes; node -1 and num_joints 0: morph weights only */
typedef struct fovpt_rig_channel {
    int32_t target;              /* node index; for FOVPT_RIG_WEIGHTS a mesh index                                          */
    int32_t path, interpolation; /* FOVPT_RIG_TRANSLATION .. FOVPT_RIG_WEIGHTS; FOVPT_RIG_STEP or FOVPT_RIG_LINEAR          */
    uint32_t num_keys;           /* 1 .. FOVPT_RIG_MAX_KEYS                                                                 */
    const float* times;          /* num_keys, host, finite, strictly ascending                                              */
    const float* values;         /* per key 3 / 4 / 3 floats; WEIGHTS: the mesh's num_targets; host, finite                 */
} fovpt_rig_channel;             /* 32 bytes */
typedef struct fovpt_rig_clip { uint32_t num_channels, _reserved; const fovpt_rig_channel* channels; } fovpt_rig_clip;   /* 16 bytes */
typedef struct fovpt_rig_desc {
    const fovpt_rig_node* nodes;       uint32_t num_nodes, _reserved0;        /* 1 .. FOVPT_RIG_MAX_NODES                  */
    const fovpt_rig_binding* bindings; uint32_t num_bindings, _reserved1;
    const fovpt_rig_clip* clips;       uint32_t num_clips, _reserved2;        /* 0 .. FOVPT_RIG_MAX_CLIPS                  */
} fovpt_rig_desc;                /* 48 bytes */
int fovpt_set_rig(fovpt_ctx* ctx, const fovpt_rig_desc* rig /* NULL: remove */);
int fovpt_update_animated(fovpt_ctx* ctx, int clip, float time, int flags /* FOVPT_UPDATE_REBUILD */);

/* ---- the cost of the hierarchy, measured on the device -----------------------------------------------------------------------
 * A refit keeps the tree's shape, so traversal slows as the motion grows (sections 13 and 16).  What to watch is
 * the SAH cost of the nodes, in binary64: with d = hi - lo of a live child entry and area = dx * dy + dy * dz + dz * dx,
 *     cost = (root + sum of the areas of node entries + 2.7 * sum of the areas of leaf entries) / root
 * root being the area of the union of the root's live entries.  The caller rebuilds (FOVPT_UPDATE_REBUILD) when
 * current / built passes its own threshold.
 *   built      measured whenever a hierarchy is adopted (fovpt_set_scene, FOVPT_UPDATE_REBUILD).
 *   updates    the refits and rebuilds issued on this scene so far, through either entry point (calls that did nothing are not
 *              counted); fovpt_set_scene sets updates = measured = 0, a rebuild sets current = built, measured = updates.
 *   watching   a context's first fovpt_hierarchy_cost switches it on for the life of the context: from then on every refit is
 *              followed by a measurement on fovpt_stream(), enqueued behind the event frames wait for.  A context that never
 *              asks issues no extra work per update.
 *   flags 0    never blocks: the newest completed measurement, (current, measured) always a pair.  measured may lag updates.
 *   COST_WAIT  if measured != updates, measures the present tree and waits for that measurement only: measured == updates.
 *   errors     FOVPT_E_INVALID: null ctx or out, unknown flag bits.  FOVPT_E_NO_SCENE: no scene.                               */
typedef struct fovpt_hierarchy_cost_info {
    double built;                /* cost of the hierarchy as last built (fovpt_set_scene, FOVPT_UPDATE_REBUILD)             */
    double current;              /* cost measured after update number `measured`                                            */
    uint64_t updates;            /* refits and rebuilds issued on this scene so far, through either entry point             */
    uint64_t measured;           /* the value of `updates` that `current` belongs to                                        */
} fovpt_hierarchy_cost_info;
#define FOVPT_COST_WAIT 1
int fovpt_hierarchy_cost(fovpt_ctx* ctx, int flags, fovpt_hierarchy_cost_info* out);

/* ---- the hierarchy rebuilt beside the frames ------------------------------------------------------------------------------------
 * FOVPT_UPDATE_REBUILD stops the frame loop for the length of a build (15.3 ms at C3, 103 ms on the street).
 * FOVPT_UPDATE_REBUILD_ASYNC builds the new hierarchy on a thread and a stream of its own while frames go on over the refit one,
 * and swaps it in later.  A hit is the minimum (t, primitive id) and occlusion is existence, so no pixel depends on which
 * conservative tree is in use: the swap is invisible bit for bit.
 *   the flag   accepted by all five fovpt_update_* calls, refused (FOVPT_E_INVALID) together with FOVPT_UPDATE_REBUILD.  The call
 *              is the call without the flag: same validation, writes, refit, event, `updates` count and stream ordering.  If the
 *              state is IDLE it then enqueues, on fovpt_stream() behind the refit, a snapshot of the current positions (9 floats
 *              per triangle into a buffer the build owns), starts one background build over it and returns; it never waits for the
 *              device.  With no entries it is a background rebuild alone (nothing moves, no refit, nothing counted; the device
 *              copies of the indices and positions are made if the scene has not been updated yet).  In state BUILDING or READY no
 *              second build starts: `requested` counts the request, `started` does not.  The state is the one the call finds
 *              when it comes in: a flagged call that finds READY and adopts (below) leaves IDLE behind and starts nothing.  One
 *              build per context is in flight.
 *              (Its value is 16: the bits 4 and 8 are refused as unknown, as they always were.)
 *   the build  fovpt_set_scene's (FOVPT_BVH, FOVPT_SPLIT, FOVPT_REINSERT, FOVPT_BVH_ORDER, and the second build without
 *              reinsertion when the first is too deep), on a host thread that owns a stream of the lowest priority the device
 *              offers, which waits for the snapshot's event.  The environment is read by the requesting call, on its thread: a
 *              caller may change it while a build runs.  The thread touches nothing of the context but its own job record; it
 *              measures the new tree's cost with partial sums of its own and publishes hierarchy, levels, scene facts, cost and
 *              build time together.  A hierarchy too deep for the traversal stack (FOVPT_E_BVH_DEPTH), of more than 64 levels or
 *              beyond the 32-bit offsets (FOVPT_E_INVALID), or a device error (FOVPT_E_DEVICE) is a failed build: nothing is kept,
 *              the present hierarchy stays, `failed` counts it, `last_error` holds the code, the state is IDLE again and a later
 *              request starts a new build.  A failed build makes no update call fail; fovpt_last_error gives its text after the
 *              next fovpt_rebuild_state.
 *   adoption   only in state READY and only in two places: at the start of a later fovpt_update_* call that enqueues something
 *              (not one that returns at "nothing happens", nor one with FOVPT_UPDATE_REBUILD), and in
 *              fovpt_rebuild_state(FOVPT_REBUILD_ADOPT).  So what fovpt_debug_buffer shows of the hierarchy changes only inside
 *              calls the caller makes.  It never synchronises: on fovpt_stream() the new hierarchy becomes the scene's (with
 *              stats.num_bvh_nodes / bvh_max_depth / bvh_bytes / tri_bytes / ms_bvh_build), a refit of it over the CURRENT
 *              positions is enqueued (the snapshot may be several updates old) with the event the next job waits for, `updates`
 *              counts 1, `built` becomes the cost the builder measured and, if the context is watching, a measurement follows as
 *              behind any refit.  Frames already issued keep reading the old hierarchy.  Its memory is retired with events
 *              recorded behind everything that can read it and released once a poll finds them complete, at a later update call
 *              that enqueues something, fovpt_rebuild_state, fovpt_set_scene or fovpt_destroy; no call waits for those events
 *              (the release itself, hipFree, waits for the device: DESIGN.md, section 27).  Positions, primitive ids, the
 *              traversable handle, the temporal history and the tracking of fovpt_temporal_motion / fovpt_warp_motion are
 *              untouched; a caller's G-buffer traced before the adoption no longer goes with the context's hit records
 *              (fovpt_warp_motion with that G-buffer: FOVPT_E_NO_FRAME, as after an update).
 *   ended      fovpt_set_scene, a FOVPT_UPDATE_REBUILD and fovpt_destroy end a background build early: the thread is joined and
 *              the result freed (`discarded` counts it).  These calls are host-synchronous already.
 *   state      fovpt_rebuild_state never waits for the device.  flags 0: polls.  FOVPT_REBUILD_WAIT: waits until the state is not
 *              BUILDING, for the builder's thread and nothing else.  FOVPT_REBUILD_ADOPT: adopts now if READY (after the wait, if
 *              both are given); in any other state it does nothing.
 *   errors     FOVPT_E_INVALID: null ctx or out, unknown flag bits.  FOVPT_E_NO_SCENE: no scene.
 * A context that never passes the flag creates no thread and no stream and issues exactly the HIP calls it issued before.
 * FOVPT_ASYNC_BUILD_DELAY_MS (tests and tuning only; read by the requesting call): the builder's thread sleeps that long before it
 * publishes.  Default 0; it changes no result.
 * Device memory: the snapshot, 40 bytes per triangle (36 of positions, 4 of the mesh index), from the first request until the next
 * fovpt_set_scene.  While a build runs, the builder's scratch on top, the same as in fovpt_set_scene: for the default build (PLOC with
 * reinsertion, no splits) about 460 bytes per triangle, added up from the sizes of its arrays (176 of them the result before it
 * is packed, 128 per binary node and 48 per triangle record; the sort's temporary storage comes on top).  From READY until the old
 * one is released, the second hierarchy (stats.bvh_bytes + stats.tri_bytes).
 * Time (MI355X; two frames in flight, a quarter of the meshes turning 3 degrees per frame, a rebuild asked
 * for at current / built > 2): an adoption is 0.12 ms of device time at C3 and 0.47 ms on the street.  A build beside the frames
 * takes 250 .. 590 ms at C3 against 15 ms on a stalled device, because every host round trip of the builder waits for frames: the
 * longest frame interval falls from 14 ms to 5 .. 7 ms, the mean rises from 2.1 to 2.5 ms (the refit tree serves longer), and a
 * fovpt_render issued while a build runs took up to 4.5 ms on the host.  On the street the build (13.5 s) does not keep up with the
 * degrading tree: there FOVPT_UPDATE_REBUILD, or a much earlier request, is the better choice.                                      */
#define FOVPT_UPDATE_REBUILD_ASYNC 16  /* all five fovpt_update_* calls; refused together with FOVPT_UPDATE_REBUILD              */
#define FOVPT_REBUILD_IDLE 0           /* nothing in flight                                                                      */
#define FOVPT_REBUILD_BUILDING 1       /* a background build is running                                                          */
#define FOVPT_REBUILD_READY 2          /* a finished hierarchy waits to be adopted                                               */
#define FOVPT_REBUILD_WAIT 1           /* flag: wait until the state is not BUILDING (and for nothing else)                      */
#define FOVPT_REBUILD_ADOPT 2          /* flag: adopt now if READY (after WAIT, if both are given)                               */
typedef struct fovpt_rebuild_info {
    int32_t state, last_error;   /* last_error: 0, or the FOVPT_E_* of the last background build that failed                */
    uint64_t requested, started, adopted, failed, discarded;
    uint64_t snapshot_update;    /* the value of fovpt_hierarchy_cost_info.updates the newest snapshot was taken at         */
    double ms_build;             /* device time of the last finished background build, on its own stream                    */
} fovpt_rebuild_info;
int fovpt_rebuild_state(fovpt_ctx* ctx, int flags, fovpt_rebuild_info* out);

/* CUDAProbeData::createBuffer (Probe.h:102-124): uploads the 5 arrays, fills *probe_out
 * with device pointers exactly as setProbe does (SimplePathtracer.cpp:292-308).   */
int fovpt_set_probe(fovpt_ctx* ctx, int width, int height, const fovpt_float4* data,
                    const float* pdfValuesX, const float* cdfValuesX,
                    const float* pdfValuesY, const float* cdfValuesY,
                    const fovpt_float3* offset, fovpt_probe* probe_out);

/* The same, with ProbeData::BuildCDF (Probe.h:29-77) done on the device: uploads only the texels and
 * builds pdf/cdf tables in HBM with the reference's left-to-right fp32 summation order (rows in
 * parallel).  Bit-identical to fovpt_probe_build_cdf + fovpt_set_probe.                          */
int fovpt_set_probe_data(fovpt_ctx* ctx, int width, int height, const fovpt_float4* data,
                         const fovpt_float3* offset, fovpt_probe* probe_out);

/* SampleRenderer::resize (SimplePathtracer.cpp:228-274): (re)allocates the five
 * full-frame buffers.  No-op returning FOVPT_OK with *out untouched when w or h is 0. */
int fovpt_resize(fovpt_ctx* ctx, int width, int height, fovpt_frame_ptrs* out);

int fovpt_get_config(const fovpt_ctx* ctx, fovpt_config* out);
int fovpt_set_config(fovpt_ctx* ctx, const fovpt_config* cfg);

/* One optixLaunch of the raygen program over a width x height grid with the given
 * parameters (SimplePathtracer.cpp:148-157).  Asynchronous on fovpt_stream().
 * With world > 1: a pixel whose last writer in THIS launch is another rank's launch index is
 * written as zero, a pixel this launch does not write is left untouched on every rank -- so a
 * frame composed of several launches (P, M, F) sums over the ranks to the single-GPU frame,
 * provided the ranks other than 0 start the frame from a cleared target (fovpt_render does
 * that clearing itself).                                                            */
int fovpt_launch(fovpt_ctx* ctx, const fovpt_launch_params* lp, uint32_t width, uint32_t height);

/* SampleRenderer::render() (SimplePathtracer.cpp:77-214): fills in the per-pass
 * fields of *lp exactly as the reference mutates its public launchParams (factor,
 * fillSize, radii, offset, redraw, samples_per_launch; ++subframe_index), and runs
 * the three passes (or the FOV_OFF pass) as ONE fused wavefront job.  Silently
 * returns FOVPT_OK when lp->frame.size.x == 0 (:81-82).  Asynchronous.            */
int fovpt_render(fovpt_ctx* ctx, fovpt_launch_params* lp);

/* ---- denoiser of the rendered frame ------------------------------------------------------------------------------------
 * New with this library, in place of the OptiX AI denoiser of the reference family (OtherProjects_01/06HelloPathtracing/
 * OptixDenoiser.{h,cpp}: init(DenoiseData{width, height, color, albedo, normal, output}) / exec() / finish(), and
 * SimplePathtracer.cpp's computeFinalPixelColors for the display pixels): an edge-avoiding a-trous wavelet filter (Dammertz et
 * al. 2010) over the denoiser guides (fovpt_config.write_guides = 1), made foveation-aware.  Each pixel is filtered according to
 * the pass that wrote it last -- the fovea (8 spp as shipped) not at all by default, the periphery (one sample per 4 x 4 block)
 * most -- with taps at multiples of its block fill, so a filled block is never averaged with its own copies.  Only + - * / max,
 * no transcendental functions: the result is defined bit for bit (tests/denoise_ref.py restates it in numpy float32).
 *   fovpt_denoise           filters the frame last issued with fovpt_render(ctx, lp) as it was rendered: its passes, gaze
 *                           and FOV_OFF flag are those of that call (the library keeps them), not lp's or the config's now,
 *                           so a caller may write the next gaze, camera or config before filtering.  out_color float4 (colour, alpha 1) and
 *                           out_rgba rgba8 (the resolve's tone map of out_color) per pixel, device pointers of frame.size; either
 *                           may be NULL = the context's own buffers (allocated on first use, reallocated by fovpt_resize, freed
 *                           by fovpt_destroy).  Pixels with 0 iterations get accum_buffer / frame_buffer's values unchanged.
 *                           Enqueued on fovpt_stream(), not synchronised: behind that frame's resolve and ahead of the next
 *                           frame's, whatever frames_in_flight / chains_per_frame say.  Reads the guides; writes nothing else.
 *                           FOVPT_E_INVALID: null arguments, an iteration count outside 0 .. 5, a sigma outside
 *                           [FOVPT_SIGMA_MIN, FOVPT_SIGMA_MAX] (or NaN), a frame rendered with write_guides = 0 (or
 *                           shadow-catcher scenes, which cannot write guides) or world > 1 (a shard has no neighbours);
 *                           FOVPT_E_NO_FRAME: nothing rendered since create / resize, or lp->frame.size differs.
 *   fovpt_denoise_buffers   addresses of the context's own outputs (allocated for the last frame if not yet).                 */
#define FOVPT_DENOISE_MAX_ITERATIONS 5
/* the accepted range of every edge-stopping scale (fovpt_denoise_config and fovpt_reconstruct_config *_sigma): 1 / sigma^2
 * stays a normal float and the denoiser's colour scale 4^(FOVPT_DENOISE_MAX_ITERATIONS - 1) / (1e-4 sigma^2) stays finite */
#define FOVPT_SIGMA_MIN 1e-6f
#define FOVPT_SIGMA_MAX 1e6f
typedef struct fovpt_denoise_config {
    int32_t iterations_fovea;      /* a-trous iterations of pixels last written by pass F (fill 1); default 0             */
    int32_t iterations_middle;     /* ... by pass M (fill 2); default 2                                                    */
    int32_t iterations_periphery;  /* ... by pass P (fill 4); default 3                                                    */
    int32_t iterations_uniform;    /* FOV_OFF frames (one pass, fill 1); default 3                                         */
    float color_sigma;             /* edge-stopping scales: colour (relative to the pixel's luminance, halved per          */
    float normal_sigma;            /* iteration), normal and albedo distance, each FOVPT_SIGMA_MIN .. FOVPT_SIGMA_MAX;    */
                                   /* defaults from fovpt_denoise_defaults                                                 */
    float albedo_sigma;
    int32_t _reserved;             /* 0 */
} fovpt_denoise_config;
int fovpt_denoise_defaults(fovpt_denoise_config* out);
int fovpt_denoise(fovpt_ctx* ctx, const fovpt_launch_params* lp, const fovpt_denoise_config* dc,
                  fovpt_float4* out_color, uint32_t* out_rgba);
int fovpt_denoise_buffers(fovpt_ctx* ctx, fovpt_float4** color, uint32_t** rgba);

/* ---- G-buffer and reconstruction of the rendered frame ---------------------------------------------------------------
 * New with this library (the reference family has no counterpart; its denoiser runs on the block-filled frame).  A foveated
 * frame leaves the periphery as 4 x 4 copies of one sample and the middle ring as 2 x 2 copies; fovpt_reconstruct rebuilds
 * those pixels from the 3 x 3 neighbouring samples of their fill, guided by a full-resolution primary-visibility G-buffer
 * (cf. Weier et al. 2016, Koskela et al. 2019), and remodulates with per-pixel albedo so that textures are sharp again.
 * Only + - * / max min: the result is defined bit for bit (tests/reconstruct_ref.py restates it in numpy float32).
 *   fovpt_gbuffer              traces one ray per pixel of lp->frame.size with lp's camera (generate_rays' expression with
 *                              jitter 0.5, the production closest-hit traversal) into buffers the context owns (allocated on
 *                              first use, reallocated by fovpt_resize, freed by fovpt_destroy); `out` receives their device
 *                              pointers.  Per pixel: prim (global primitive id, 0xffffffff on a miss), position (eye + t dir,
 *                              t; a miss (0, 0, 0, -1)), normal (the face-forwarded geometric normal of the shading kernel, w 0)
 *                              and albedo (material colour or its texel, w 0); a miss has zero normal and albedo.  Enqueued on
 *                              fovpt_stream(), not synchronised.  FOVPT_E_INVALID: null arguments, an empty frame size;
 *                              FOVPT_E_NO_SCENE: no scene (or lp->traversable is not the current one).
 *   fovpt_reconstruct          reconstructs the frame last issued with fovpt_render(ctx, lp) as it was rendered: its passes,
 *                              gaze and camera are those of that call, not lp's or the config's now.  Builds its G-buffer
 *                              (that camera, lp->frame.size), then for
 *                              every pixel whose last writer has fill f > 1 and whose level is on in rc->levels, interpolates
 *                              in_color / albedo guide (remodulate = 1) or in_color (0) over the 3 x 3 samples around its
 *                              block's anchor, weighted by a tent of width support * f, normal and plane-distance edge
 *                              stopping, and multiplies by the pixel's own G-buffer albedo.  in_color NULL = accum_buffer
 *                              (typically: fovpt_denoise's colour output otherwise).  Other pixels, and pixels whose weights
 *                              sum to 0, get in_color unchanged.  out_color float4 (alpha 1 where reconstructed), out_rgba
 *                              rgba8 (the resolve's tone map of out_color), device pointers of frame.size; either may be NULL
 *                              = the context's own buffers.  Enqueued on fovpt_stream(), not synchronised, ordered like
 *                              fovpt_denoise.  Writes its outputs and the G-buffer, nothing else.  FOVPT_E_INVALID: null
 *                              ctx / lp / rc, a value out of range (a sigma outside [FOVPT_SIGMA_MIN, FOVPT_SIGMA_MAX]),
 *                              remodulate = 1 on a frame rendered with write_guides = 0 (or shadow-catcher scenes), a frame
 *                              rendered with world > 1, in_color equal to the output colour buffer; FOVPT_E_NO_SCENE: no scene;
 *                              FOVPT_E_NO_FRAME: nothing rendered since create / resize, or lp->frame.size differs.
 *   fovpt_reconstruct_buffers  addresses of the context's own outputs (allocated for the last frame if not yet).        */
typedef struct fovpt_gbuffer_ptrs {
    uint32_t* prim;                /* device pointers, width * height entries each                                          */
    fovpt_float4* position;
    fovpt_float4* normal;
    fovpt_float4* albedo;
    int32_t width, height;
} fovpt_gbuffer_ptrs;
typedef struct fovpt_reconstruct_config {
    float support;                 /* tent half-width in samples of the fill, 1 .. 2; default 2                             */
    float normal_sigma;            /* normal edge stopping, FOVPT_SIGMA_MIN .. MAX; default 0.5                            */
    float depth_sigma;             /* plane-distance edge stopping relative to the pixel's t, FOVPT_SIGMA_MIN .. MAX; 0.05 */
    int32_t levels;                /* bit 0: middle ring (fill 2), bit 1: periphery (fill 4); default 3                     */
    int32_t remodulate;            /* 1: interpolate colour / albedo guide, multiply by the G-buffer albedo; default 1      */
    int32_t _reserved[3];          /* 0 */
} fovpt_reconstruct_config;
int fovpt_gbuffer(fovpt_ctx* ctx, const fovpt_launch_params* lp, fovpt_gbuffer_ptrs* out);
int fovpt_reconstruct_defaults(fovpt_reconstruct_config* out);
int fovpt_reconstruct(fovpt_ctx* ctx, const fovpt_launch_params* lp, const fovpt_reconstruct_config* rc, const fovpt_float4* in_color,
                      fovpt_float4* out_color, uint32_t* out_rgba);
int fovpt_reconstruct_buffers(fovpt_ctx* ctx, fovpt_float4** color, uint32_t** rgba);

/* ---- temporal reprojection of the frame history ----------------------------------------------------------------------
 * New with this library (the reference family's only temporal mechanism is accumulate = 1, correct for a static camera
 * alone).  Carries a per-pixel history from one rendered frame to the next while the camera and gaze move: each pixel's
 * primary hit (a miss: its ray direction) is projected into the previous step's camera, the previous history is read there
 * with bilinear weights over the taps whose previous G-buffer agrees with the pixel's, and blended with the new frame as a
 * running mean of at most `cap` frames, cap chosen by the pixel's foveation level.  No clamp to the current neighbourhood:
 * with one sample per 4 x 4 block it is noise; the caps bound ghosting instead.  Only + - * / min floor and comparisons:
 * the result is defined bit for bit (tests/temporal_ref.py restates it in numpy float32).
 *   fovpt_temporal           one step of the context's history, on the frame last issued with fovpt_render(ctx, lp) as it
 *                            was rendered (its passes, gaze and camera, not lp's or the config's now).  Traces that frame's
 *                            G-buffer (as fovpt_gbuffer, into buffers of its own: fovpt_gbuffer's keep their contents), then
 *                            per pixel p with hit point X_p, t_p, normal N_p:
 *                              cap N      history_periphery / _middle / _fovea by the fill (4 / 2 / 1) of the pixel's last
 *                                         writer, history_uniform on a FOV_OFF frame, 1 where no pass writes
 *                              project    v = X_p - eye_prev (a miss: dx U + dy V + W, its ray before normalising);
 *                                         a = inverse(U_prev V_prev W_prev) v (inverse in binary64, entries rounded to fp32);
 *                                         a.z > 0, px = ((a.x / a.z + 1) * 0.5) * w - 0.5 in [-1, w), py likewise
 *                              taps       the 4 bilinear taps around (px, py) in the frame, of p's class (both misses or both
 *                                         hits) and, for hits, |N_q - N_p|^2 <= normal_tolerance and
 *                                         |N_p . (X_q - X_p)| <= depth_tolerance * t_p on the previous G-buffer
 *                              history    sum w >= 1/64: H = sum w H_q / sum w, n_h = sum w n_q / sum w; else n_h = 0
 *                              blend      n = min(n_h + 1, N); n == 1: out = in_color bit for bit; else
 *                                         out = H + (1 / n) (in - H), alpha 1
 *                            and the new history (out, n).  in_color NULL = accum_buffer (typically fovpt_reconstruct's or
 *                            fovpt_denoise's colour output otherwise); out_color may equal in_color (a pixel reads only
 *                            itself of the input).  out_color float4, out_rgba rgba8 (the resolve's tone map of out_color),
 *                            device pointers of frame.size; either may be NULL = the context's own buffers.  Enqueued on
 *                            fovpt_stream(), not synchronised, ordered like fovpt_denoise.  The first step, and the first
 *                            after fovpt_temporal_reset, fovpt_resize or fovpt_set_scene, has no history: out = in_color,
 *                            n = 1.  fovpt_set_probe keeps the history: a caller that changes the lighting calls
 *                            fovpt_temporal_reset.  FOVPT_E_INVALID: null ctx / lp / tc, a value out of range (NaN
 *                            included), non-zero reserved fields, a frame rendered with world > 1, out_color equal to the
 *                            context's history; FOVPT_E_NO_SCENE: no scene (or lp->traversable is not the current one);
 *                            FOVPT_E_NO_FRAME: nothing rendered since create / resize, or lp->frame.size differs.
 *   fovpt_temporal_buffers   addresses of the context's own outputs and of the history the last call wrote (rgb = its
 *                            output colour, w = n); allocated for the last frame if not yet.
 *   fovpt_temporal_reset     drops the history: the next call starts a new one.
 * Defaults chosen by measurement: on a 12-frame camera path they cut the periphery's RMSE against a
 * 256-spp render 1.95x over fovpt_reconstruct alone, the middle ring's 1.42x, and leave the fovea as it is.  On an MI355X a
 * call takes 0.29 ms at 1920 x 1080, of which 0.09 ms is the reprojection and the rest its G-buffer.                      */
#define FOVPT_TEMPORAL_MAX_HISTORY 64
typedef struct fovpt_temporal_config {
    int32_t history_fovea;         /* cap on the history length of pixels last written by pass F (fill 1), 1 .. MAX; 1      */
    int32_t history_middle;        /* ... pass M (fill 2); default 4                                                          */
    int32_t history_periphery;     /* ... pass P (fill 4); default 8                                                          */
    int32_t history_uniform;       /* FOV_OFF frames; default 4                                                               */
    float normal_tolerance;        /* |N_q - N_p|^2 <= this keeps a tap, 0 .. 4; default 0.1                                  */
    float depth_tolerance;         /* |N_p . (X_q - X_p)| <= this * t_p keeps a tap, 0 .. 1; default 0.02                     */
    int32_t _reserved[2];          /* 0 */
} fovpt_temporal_config;
int fovpt_temporal_defaults(fovpt_temporal_config* out);
int fovpt_temporal(fovpt_ctx* ctx, const fovpt_launch_params* lp, const fovpt_temporal_config* tc, const fovpt_float4* in_color,
                   fovpt_float4* out_color, uint32_t* out_rgba);
int fovpt_temporal_buffers(fovpt_ctx* ctx, fovpt_float4** color, uint32_t** rgba, const fovpt_float4** history);
int fovpt_temporal_reset(fovpt_ctx* ctx);
/* ---- the temporal step for animated scenes: moved meshes are reprojected by their own motion -------------------------------
 *   fovpt_temporal_motion    fovpt_temporal -- the same config, validation, error codes, context-owned outputs, stream and
 *                            ordering, and the SAME history and G-buffer sets: a caller may mix the two calls -- except that a
 *                            hit pixel p on a mesh that fovpt_update_vertices has moved since the previous temporal step (through
 *                            either call; refit or FOVPT_UPDATE_REBUILD, host or device pointers) takes its point and normal
 *                            where the surface was when that step ran.  With the hit's barycentrics (u, v), a', b', c' the
 *                            positions its triangle's vertices had then (in the order of the mesh's index triple), every
 *                            operation one unfused binary32 operation per component:
 *                              w0 = (1 - u) - v;  X' = (w0 a' + u b') + v c';  N' = normalize(cross(b' - a', c' - a')) * s,
 *                              s = +-1 as the G-buffer face-forwarded p's current normal
 *                            and the step is fovpt_temporal's with X' for X_p and N' for N_p (t_p stays the current one).
 *                            Pixels of meshes that have not moved, and misses, are fovpt_temporal's bit for bit.  A degenerate
 *                            previous triangle has no normal: the pixel starts a new history (n = 1).
 *                            tests/temporal_motion_ref.py restates it in numpy float32.
 *                            out_motion (may be NULL): float4 per pixel of frame.size, for every pixel whatever its cap:
 *                            (px - x, py - y, a.z, 1) where the pixel reprojects (a.z > 0, -1 <= px < w, -1 <= py < h: the
 *                            pixel was at (x + .x, y + .y) in the previous step's frame, .z its depth along the previous W), and
 *                            (0, 0, 0, 0) where it does not, and everywhere on a step without history.  It must be none of the
 *                            call's other buffers and not the context's history (FOVPT_E_INVALID).
 *   previous positions       A context's first fovpt_temporal_motion (and the first after fovpt_set_scene) switches tracking on:
 *                            from then on fovpt_update_vertices copies a mesh's positions aside (12 bytes per vertex, on the
 *                            device, in stream order ahead of the new positions) the first time it moves the mesh after a
 *                            temporal step.  Every temporal step through either call ends that interval.  If an update ran
 *                            since the previous step while tracking was still off, that fovpt_temporal_motion step has no
 *                            history, as after fovpt_temporal_reset.  A context that never calls fovpt_temporal_motion pays
 *                            nothing.
 *   the loop                 update_vertices -> render -> (denoise, reconstruct) -> temporal_motion -> update_vertices ...
 *                            The step traces its G-buffer when it is called, so the caller steps BEFORE it moves the meshes
 *                            for the next frame (as with fovpt_temporal).
 * Reflections and shadows of moving objects are not reprojected by that motion: the caps bound their lag.  On an MI355X at
 * 1920 x 1080 a step takes 0.003 ms more than fovpt_temporal's (0.006 ms with motion vectors), and tracking adds 0.012 ms to
 * an update of 140 k vertices, 0.031 ms to one of 2.6 M.                                           */
int fovpt_temporal_motion(fovpt_ctx* ctx, const fovpt_launch_params* lp, const fovpt_temporal_config* tc, const fovpt_float4* in_color,
                          fovpt_float4* out_color, uint32_t* out_rgba, fovpt_float4* out_motion /* may be NULL */);

/* ---- the post-frame chain in one call ------------------------------------------------------------------------------------
 *   fovpt_post               "make the frame I just rendered displayable": the enabled stages of
 *                              DENOISE      fovpt_denoise(ctx, lp, &pc->denoise, NULL, NULL): into the context's denoise buffers
 *                                           (fovpt_denoise_buffers) -- or, when it is the only stage, into this call's outputs
 *                              RECONSTRUCT  fovpt_reconstruct of the denoiser's colour output if DENOISE is on, of in_color
 *                                           otherwise (NULL = accum_buffer)
 *                              TEMPORAL     fovpt_temporal -- with MOTION fovpt_temporal_motion -- of the previous enabled
 *                                           stage's colour output, or of in_color if there is none
 *                            made one after the other on the frame last issued with fovpt_render(ctx, lp): every output, and all
 *                            state the call leaves behind, is bit for bit what those calls give.  The history, the two G-buffer
 *                            sets and the tracking of previous positions are the temporal calls' own, so a caller may mix
 *                            fovpt_post, fovpt_temporal and fovpt_temporal_motion steps on one context.  out_color, out_rgba and
 *                            out_motion (MOTION only) are the last enabled stage's outputs; out_color / out_rgba NULL = the
 *                            context's own post buffers (fovpt_post_buffers: allocated on first use, reallocated by
 *                            fovpt_resize, freed by fovpt_destroy).  Enqueued on fovpt_stream(), not synchronised, ordered like
 *                            fovpt_denoise.
 *                            What differs from making the calls: with RECONSTRUCT and TEMPORAL both on, the frame's G-buffer is
 *                            traced ONCE, into the temporal step's set, the reconstruction reads that set, and its colour goes
 *                            from one stage to the next in registers (one kernel for both): the reconstruction's colour is
 *                            written nowhere, and fovpt_reconstruct_buffers and the buffers fovpt_gbuffer hands out keep their
 *                            contents.  That kernel reads in_color and the albedo guide across pixels while it writes, so no
 *                            output and neither history may be one of them (FOVPT_E_INVALID).  Every other combination is the
 *                            stage calls' own launches.
 *                            All or nothing: every stage is checked before anything is enqueued or any state moves.  Error codes
 *                            are the stage calls' own (ranges, reserved fields, world > 1, FOVPT_E_NO_SCENE, FOVPT_E_NO_FRAME,
 *                            write_guides for DENOISE and for remodulate = 1), and FOVPT_E_INVALID for: null ctx / lp / pc;
 *                            stages 0 or with unknown bits; MOTION without TEMPORAL; out_motion without MOTION; in_color with
 *                            DENOISE (the denoiser reads accum); non-zero _reserved; with RECONSTRUCT, out_color equal to the
 *                            reconstruction's input (it reads neighbours); out_color or out_motion aliasing the history or each
 *                            other, as in fovpt_temporal_motion.
 *   fovpt_post_defaults      RECONSTRUCT | TEMPORAL | MOTION, each stage's config its own defaults.
 *   fovpt_post_buffers       addresses of the context's own post outputs (allocated for the last frame if not yet).
 * On an MI355X at 1920 x 1080 the default chain takes 0.39 ms, against 0.62 ms for fovpt_reconstruct followed by
 * fovpt_temporal_motion.                                                                          */
#define FOVPT_POST_DENOISE      1
#define FOVPT_POST_RECONSTRUCT  2
#define FOVPT_POST_TEMPORAL     4
#define FOVPT_POST_MOTION       8   /* the temporal stage is fovpt_temporal_motion's; needs FOVPT_POST_TEMPORAL */
typedef struct fovpt_post_config {
    int32_t stages;                       /* FOVPT_POST_* bits; default RECONSTRUCT | TEMPORAL | MOTION */
    int32_t _reserved[3];                 /* 0 */
    fovpt_denoise_config denoise;         /* each the stage call's own config, with its own defaults */
    fovpt_reconstruct_config reconstruct;
    fovpt_temporal_config temporal;
} fovpt_post_config;
int fovpt_post_defaults(fovpt_post_config* out);
int fovpt_post(fovpt_ctx* ctx, const fovpt_launch_params* lp, const fovpt_post_config* pc, const fovpt_float4* in_color,
               fovpt_float4* out_color, uint32_t* out_rgba, fovpt_float4* out_motion /* may be NULL */);
int fovpt_post_buffers(fovpt_ctx* ctx, fovpt_float4** color, uint32_t** rgba);

/* ---- gaze-metered auto-exposure and tone map -------------------------------------------------------------------------------
 * New with this library: every other stage writes its rgba8 as make_color(reinhard(c * 16, 1)), the constants of the reference's
 * shipped app.  fovpt_expose is the stage behind them (typically fed fovpt_post's colour output) with an exposure that follows
 * what the eye looks at: meter -> adapt -> apply, all on the device in stream order, no host synchronisation.
 *   fovpt_expose             works on the frame last issued with fovpt_render(ctx, lp) as it was rendered (its passes, gaze and
 *                            FOV_OFF flag).  in_color NULL = accum_buffer; out_color / out_rgba NULL = the context's own buffers
 *                            (fovpt_expose_buffers: allocated on first use, reallocated by fovpt_resize, freed by fovpt_destroy).
 *                            out_color may be in_color (the meter has finished before any pixel is written, and a pixel reads only
 *                            itself).  Enqueued on fovpt_stream(), not synchronised, ordered like fovpt_denoise.  Writes its
 *                            outputs, the exposure state and its own scratch, nothing else.  The definition, operation by
 *                            operation (tests/expose_ref.py), every fp32 *, + and / one unfused operation:
 *                              1 luminance   L = (0.2126f * r + 0.7152f * g) + 0.0722f * b of in_color
 *                              2 bin         a pixel counts if L > 0 (+inf counts; NaN, 0, negatives do not); with u the bits of L,
 *                                            bin = clamp((u >> 20) - 888, 0, 255): 8 bins per octave over 2^-16 .. 2^16
 *                              3 histogram   h[bin] += weight(pixel), integer weights, 64-bit totals.  METER_FRAME: 1 for every
 *                                            pixel.  METER_GAZE: weight_fovea / _middle / _periphery by the fill (1 / 2 / 4) of
 *                                            the pixel's last writer, weight_uniform on a FOV_OFF frame, 0 where no pass writes
 *                              4 trimmed mean  T = sum h, a = T * low / 1000, b = (T * high + 999) / 1000 (integer division),
 *                                            N = b - a; with cum the running sum c_k = max(0, min(cum[k+1], b) - max(cum[k], a)),
 *                                            S = sum c_k (2k + 1) in 64-bit integers;
 *                                            ev_metered = (float)clamp(-16.0 + ((double)S / (2.0 * (double)N)) / 8.0, ev_min, ev_max);
 *                                            N == 0: the present ev (on a first step clamp(0, ev_min, ev_max))
 *                              5 adapt       first step after create / reset: ev = ev_metered; otherwise
 *                                            ev = ev + a * (ev_metered - ev), a = adapt_brighter if ev_metered > ev else adapt_darker
 *                              6 exposure    E = key / fovpt_dm_powf(2.0f, ev)
 *                              7 apply       o = tone(c.rgb, E), out_color = (o, 1), out_rgba = make_color(o).  TONE_REINHARD is
 *                                            the resolve's reinhard(c * E, white) (so FIXED, exposure 16, REINHARD, white 1 gives
 *                                            the rgba8 of the other stages bit for bit); TONE_ACES per channel with x = c * E:
 *                                            (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f).  Outputs for input
 *                                            pixels that are non-finite or negative are unspecified.
 *                            EXPOSE_FIXED: E = cfg.exposure, step 7 alone; nothing is metered, the state is untouched.
 *                            The state survives fovpt_resize and fovpt_set_probe; fovpt_expose_reset and fovpt_set_scene reset it.
 *                            All or nothing, checked before anything is enqueued.  FOVPT_E_INVALID: null ctx / lp / ec; unknown
 *                            mode, metering or tone; a weight outside 0 .. 255; permille not 0 <= low < high <= 1000; ev bounds
 *                            outside [-16, 16], out of order or NaN; key, exposure or white outside [FOVPT_SIGMA_MIN,
 *                            FOVPT_SIGMA_MAX] or NaN; an adapt rate outside (0, 1] or NaN; non-zero reserved fields; a null
 *                            input; a frame rendered with world > 1 (a shard does not see the frame).  FOVPT_E_NO_FRAME: nothing
 *                            rendered since create / resize, or lp->frame.size differs.
 *   fovpt_expose_defaults    host only, no context.  CONVENTIONS, NOT MEASUREMENTS: AUTO, METER_GAZE, REINHARD with white 1e6
 *                            (about plain x / (1 + L)), key 0.18, permille 100 .. 950, ev range -12 .. 12, both adapt rates 1
 *                            (the caller derives 1 - exp(-dt / tau) from its own frame time), FIXED's exposure 16, weights 64 / 8 / 1 / 1 (at the
 *                            shipped radii 74 / 241 on 1920 x 1080 the three levels get about a third of the weight each).
 *   fovpt_expose_buffers     addresses of the context's own exposed outputs (allocated for the last frame if not yet).
 *   fovpt_expose_state       synchronises fovpt_stream() and copies the state record out.  The struct and the function share their
 *                            name, so the struct has no typedef: write `struct fovpt_expose_state` (C and C++ alike).
 *   fovpt_expose_reset       the next AUTO step is a first step.  Enqueued on fovpt_stream().
 * On an MI355X at 1920 x 1080 a FIXED call takes 0.020 ms (fovpt_denoise with no iterations, the same traffic: 0.034 ms), an
 * AUTO call 0.045 ms with METER_FRAME and 0.063 ms with METER_GAZE: 3.1 times FIXED, 0.018 ms of it the writer search and 0.013 ms
 * k_expose_adapt.                                                                                                              */
#define FOVPT_EXPOSE_FIXED 0      /* exposure = cfg.exposure; nothing is metered, the state is untouched */
#define FOVPT_EXPOSE_AUTO  1
#define FOVPT_METER_FRAME  0      /* every pixel of the frame has weight 1 */
#define FOVPT_METER_GAZE   1      /* weight by the fill of the pixel's last writer; a pixel no pass writes: 0 */
#define FOVPT_TONE_REINHARD 0     /* the resolve's: reinhard(c * E, white) */
#define FOVPT_TONE_ACES     1     /* per channel x = c * E: (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f) */
#define FOVPT_EXPOSE_BINS 256
typedef struct fovpt_expose_config {      /* 80 bytes */
    int32_t mode, metering, tone, _reserved0;
    int32_t weight_fovea, weight_middle, weight_periphery, weight_uniform;  /* 0 .. 255; fill 1 / 2 / 4; FOV_OFF frames */
    int32_t low_permille, high_permille;  /* the ranks of the histogram that are averaged: 0 <= low < high <= 1000 */
    float ev_min, ev_max;                 /* clamp on the metered log2 luminance, -16 <= ev_min <= ev_max <= 16 */
    float key;                            /* AUTO: E = key / 2^ev */
    float exposure;                       /* FIXED: E */
    float white;                          /* REINHARD */
    float adapt_brighter, adapt_darker;   /* share of the way ev moves per step when the target is above / below it, (0, 1] */
    int32_t _reserved[3];
} fovpt_expose_config;
struct fovpt_expose_state {               /* 32 bytes */
    float ev_metered, ev, exposure, _pad;
    uint64_t weight_total;                /* T of the last metered step */
    uint64_t steps;                       /* AUTO steps since create / reset */
};
int fovpt_expose_defaults(fovpt_expose_config* out);
int fovpt_expose(fovpt_ctx* ctx, const fovpt_launch_params* lp, const fovpt_expose_config* ec, const fovpt_float4* in_color,
                 fovpt_float4* out_color, uint32_t* out_rgba);
int fovpt_expose_buffers(fovpt_ctx* ctx, fovpt_float4** color, uint32_t** rgba);
int fovpt_expose_state(fovpt_ctx* ctx, struct fovpt_expose_state* out);
int fovpt_expose_reset(fovpt_ctx* ctx);

/* ---- HDR glare ("bloom") ahead of the tone map ----------------------------------------------------------------------------------
 * New with this library.  fovpt_expose compresses everything above the display range to white; fovpt_bloom is the stage ahead of it
 * (behind fovpt_focus) that lets a highlight say how far above white it was: a thresholded, downsampled and re-expanded copy of the
 * frame added onto it, in HDR.  Two things are this renderer's own: the bright pass can weight its samples by 1 / (1 + L) (KARIS: a
 * block-filled 1-spp firefly of the periphery does not become a blob) and by a gain per foveation level (GAINS), and the threshold
 * follows the exposure, which with EXPOSURE_STATE is read from fovpt_expose's device record on the device, in stream order.
 *   fovpt_bloom              works on the frame last issued with fovpt_render(ctx, lp) as it was rendered (its size, passes, gaze and
 *                            FOV_OFF flag).  in_color NULL = accum_buffer; out_color / out_rgba NULL = the context's own buffers
 *                            (fovpt_bloom_buffers: allocated on first use with the pyramid, reallocated by fovpt_resize, freed by
 *                            fovpt_destroy).  out_color may be in_color (the pyramid is finished before any pixel is written, and the
 *                            composite reads only its own input pixel).  Enqueued on fovpt_stream(), not synchronised, ordered like
 *                            fovpt_denoise.  Writes its outputs and the pyramid, nothing else.  The definition, operation by
 *                            operation (tests/bloom_ref.py), every fp32 + - * / one unfused operation, min(a, b) = a < b ? a : b and
 *                            max likewise; w x h the frame, n = levels, level k of W_k x H_k texels with W_k = ceil(W_{k-1} / 2),
 *                            W_{-1} = w (never below 1: a 1 x 1 level is downsampled to 1 x 1 by the same rule):
 *                              0 constants   E = cfg.exposure; with EXPOSURE_STATE the exposure of fovpt_expose's state record if its
 *                                            steps != 0.  T = threshold / E, K = knee / E, K2 = 2.0f * K, K4 = 4.0f * K
 *                              1 bright pass d_0(X, Y) from the source pixels (min(2X + i, w - 1), min(2Y + j, h - 1)), j = 0, 1
 *                                            outer, i = 0, 1 inner; with c the pixel's rgb:
 *                                              L = (0.2126f * r + 0.7152f * g) + 0.0722f * b
 *                                              s = max(0, min(L - (T - K), K2));  q = K > 0 ? (s * s) / K4 : 0
 *                                              m = max(max(q, L - T), 0) / max(L, 1e-6f)
 *                                              kw = KARIS ? 1.0f / (1.0f + L) : 1.0f
 *                                              g = 1; with GAINS gain_fovea / _middle / _periphery by the fill (1 / 2 / 4) of the
 *                                                  pixel's last writer, gain_uniform on a FOV_OFF frame, 0 where no pass writes
 *                                              wt = g * kw;  num.c = num.c + wt * (c.c * m);  den = den + kw
 *                                            then d_0.c = num.c / den
 *                              2 downsample  d_k(X, Y), k = 1 .. n - 1: taps j = 0 .. 3 outer, i = 0 .. 3 inner, of
 *                                            d_{k-1}(clamp(2X - 1 + i, 0, W_{k-1} - 1), clamp(2Y - 1 + j, 0, H_{k-1} - 1)) with weight
 *                                            (float)(b_j * b_i) * 0.015625f, b = {1, 3, 3, 1}: acc.c = acc.c + weight * S.c from 0
 *                              3 upsample    up(S)(x, y) of a level S (Ws x Hs) onto a grid twice as fine: ax = x >> 1,
 *                                            bx = clamp((x & 1) ? ax + 1 : ax - 1, 0, Ws - 1), the same in y;
 *                                            r0 = 0.75f * S(ax, ay) + 0.25f * S(bx, ay), r1 = 0.75f * S(ax, by) + 0.25f * S(bx, by),
 *                                            up = 0.75f * r0 + 0.25f * r1, per channel
 *                              4 combine     u_{n-1} = d_{n-1}; k = n - 2 .. 0: u_k.c = d_k.c + spread * up(u_{k+1})(x, y).c
 *                              5 composite   B = up(u_0)(x, y); out_color = (in.r + intensity * B.r, in.g + intensity * B.g,
 *                                            in.b + intensity * B.b, in.w); out_rgba = make_color(reinhard(out.rgb * 16, 1)), as in
 *                                            every stage
 *                            Outputs for input colours that are non-finite or negative are unspecified.  A non-negative frame whose
 *                            every L <= T - K comes back bit for bit, at any intensity.  The pyramid is one allocation of float4
 *                            texels (the fourth channel 0), the levels packed one after the other; u_k overwrites d_k, and after a
 *                            call every level's u_k is in memory (fovpt_debug_buffer "bloom_pyramid").
 *                            All or nothing, checked before anything is enqueued.  FOVPT_E_INVALID: null ctx / lp / bc; unknown
 *                            flag bits; levels outside 1 .. FOVPT_BLOOM_MAX_LEVELS; threshold or exposure outside [FOVPT_SIGMA_MIN,
 *                            FOVPT_SIGMA_MAX] or NaN; knee or intensity outside [0, FOVPT_SIGMA_MAX] or NaN; spread or a gain outside
 *                            [0, 1] or NaN; non-zero reserved fields; a null input; width * height >= 2^31; out_color or out_rgba
 *                            the pyramid or each other, out_rgba or the pyramid the input; a frame rendered with world > 1 (a shard
 *                            does not see the frame).  FOVPT_E_NO_FRAME: nothing rendered since create / resize, or lp->frame.size
 *                            differs.
 *   fovpt_bloom_defaults     host only, no context.  CONVENTIONS, NOT MEASUREMENTS: KARIS only, 6 levels, threshold 1, knee 0.5,
 *                            exposure 16 (the shipped app's constant), intensity 0.05, spread 0.7, all gains 1.
 *   fovpt_bloom_buffers      addresses of the context's own outputs (allocated for the last frame if not yet).
 * On an MI355X at 1920 x 1080 a call at the defaults takes 0.067 ms, 3.3 times fovpt_expose FIXED (a plain full-frame pass: 0.020 ms)
 * measured beside it; with GAINS 0.088 ms (four writer searches per texel of the first level), with 8 levels 0.075 ms; one
 * fovpt_render 0.68 ms.  Every level is one launch: one workgroup making the small levels in LDS measured slower at the defaults, and
 * the composite's once-written outputs are nt stores, which measured no worse (EXPERIMENTS.md).               */
#define FOVPT_BLOOM_MAX_LEVELS 8
#define FOVPT_BLOOM_KARIS          1   /* flags: weight the first downsample's samples by 1 / (1 + L) */
#define FOVPT_BLOOM_GAINS          2   /* per-level gains by the last writer's fill; off: gain 1 everywhere, no writer search */
#define FOVPT_BLOOM_EXPOSURE_STATE 4   /* E from fovpt_expose's device record (steps != 0), else cfg.exposure */
typedef struct fovpt_bloom_config {    /* 64 bytes */
    int32_t flags, levels;             /* levels 1 .. FOVPT_BLOOM_MAX_LEVELS */
    float threshold, knee;             /* in exposed units: compared against L * E */
    float exposure;                    /* E unless EXPOSURE_STATE applies */
    float intensity, spread;
    float gain_fovea, gain_middle, gain_periphery, gain_uniform;
    int32_t _reserved[5];
} fovpt_bloom_config;
int fovpt_bloom_defaults(fovpt_bloom_config* out);
int fovpt_bloom(fovpt_ctx* ctx, const fovpt_launch_params* lp, const fovpt_bloom_config* bc, const fovpt_float4* in_color /* NULL: accum_buffer */,
                fovpt_float4* out_color, uint32_t* out_rgba /* NULL: the context's own */);
int fovpt_bloom_buffers(fovpt_ctx* ctx, fovpt_float4** color, uint32_t** rgba);

/* ---- late reprojection ("timewarp") of a finished frame to a newer camera ----------------------------------------------------
 * New with this library.  A head-mounted or gaze-tracked client learns its newest camera pose after fovpt_render was issued (with
 * two frames in flight it is two poses behind): fovpt_warp re-aims the finished image at that pose just before display.
 * fovpt_temporal pulls old colours into a new frame whose depth is known, a gather; here only the OLD frame's depth is known, so
 * the stage is a depth-tested forward scatter (k_warp_scatter) followed by a resolve that closes cracks and disocclusions from the
 * farthest surface nearby (k_warp_resolve).  No arithmetic touches a colour: a pixel is copied, so the result is defined bit for bit.
 *   fovpt_warp               works on the frame last issued with fovpt_render(ctx, lp) as it was rendered: its size and camera (the
 *                            camera is needed only for the directions of miss pixels).  `to`: the camera to warp to, in
 *                            LaunchParams.camera's layout.  gbuffer NULL: the call traces the rendered camera's G-buffer into
 *                            fovpt_gbuffer's buffers, exactly as fovpt_reconstruct does (so it needs the scene); non-NULL: the
 *                            pointers are used as given, only prim and position are read, and the caller vouches that they belong
 *                            to the frame -- with fovpt_temporal_gbuffer's set the loop render -> post -> expose ->
 *                            temporal_gbuffer -> warp traces one G-buffer per frame, not two.  in_color NULL = accum_buffer,
 *                            in_rgba NULL = frame_buffer (typically fovpt_expose's outputs); out_color / out_rgba NULL = the
 *                            context's own (fovpt_warp_buffers: allocated on first use together with an 8-byte-per-pixel key
 *                            buffer, reallocated by fovpt_resize, freed by fovpt_destroy; a context that never warps pays
 *                            nothing); out_map (may be NULL): uint32 per pixel, source | class << 30.  Only the images of
 *                            cfg.images are read and written.  The outputs are written whole.  Enqueued on fovpt_stream(), not
 *                            synchronised, ordered like fovpt_denoise.  The definition, operation by operation
 *                            (tests/warp_ref.py), every fp32 *, +, - and / one unfused operation; w, h the frame size,
 *                            s = y * w + x a source pixel, M the rows of inverse(U V W) of `to` as fovpt_temporal computes the
 *                            previous camera's (binary64, entries rounded to fp32):
 *                              scatter     v = X_s - eye_to for a hit (prim != 0xffffffff), (dx U + dy V) + W of the rendered
 *                                          camera for a miss (the sky is at infinity: only rotation moves it);
 *                                          a_k = (M_k.x v.x + M_k.y v.y) + M_k.z v.z;
 *                                          px = (((a.x / a.z) + 1) * 0.5) * w - 0.5, py likewise with h;
 *                                          fx = floor(px + 0.5f), fy likewise; the pixel lands iff a.z > 0, 0 <= fx < w and
 *                                          0 <= fy < h (compared in float: NaNs fall out); depth word d = the bits of a.z for a
 *                                          hit, 0x7fffffff for a miss; key = d << 32 | s;
 *                                          keys[fy * w + fx] = min(keys[...], key), keys all ones before.  Nearest depth wins,
 *                                          equal depths go to the lower source index, whatever the arrival order
 *                              resolve     per destination pixel q.  Key not empty: class direct (0), the source is the key's
 *                                          low word.  Empty: for r = 1 .. fill_radius the pixels at Chebyshev distance exactly r
 *                                          inside the frame; the first r with a non-empty key ends the search, the source is
 *                                          the low word of the LARGEST key of that ring -- the farthest surface, which is what a
 *                                          disocclusion uncovers; the smallest ring keeps a crack's fill local --, class filled
 *                                          (1).  Still empty: class empty (2), the source is q itself.
 *                                          out_color[q] = in_color[src] (all four components), out_rgba[q] = in_rgba[src],
 *                                          out_map[q] = src | class << 30
 *                            All or nothing, checked before anything is enqueued.  FOVPT_E_INVALID: null ctx / lp / to / wc;
 *                            images 0 or with unknown bits; fill_radius outside 0 .. FOVPT_WARP_MAX_RADIUS; non-zero reserved
 *                            fields; a non-finite entry of `to`, or a `to` whose [U V W] has a determinant of 0 or a non-finite
 *                            one; a gbuffer whose size is not the frame's or with a null prim or position; width * height >=
 *                            2^30 (the map's class bits); an enabled image with a null input; any output equal to any input or
 *                            to another output (the resolve gathers across pixels; base addresses are compared: buffers that
 *                            overlap part of the way are the caller's to avoid); a frame rendered with world > 1.
 *                            FOVPT_E_NO_FRAME, FOVPT_E_NO_SCENE: as fovpt_reconstruct (the scene only where the call traces).
 *   fovpt_warp_defaults      host only, no context: both images, fill_radius 2 (a convention, not a measurement).
 *   fovpt_warp_buffers       addresses of the context's own warped outputs (allocated for the last frame if not yet).
 *   fovpt_warp_counts        synchronises fovpt_stream() and copies the counts of the last fovpt_warp out; zeros before any warp.
 *                            The struct and the function share their name, so the struct has no typedef: write
 *                            `struct fovpt_warp_counts` (C and C++ alike).
 *   fovpt_temporal_gbuffer   the G-buffer set the last temporal step (fovpt_temporal, fovpt_temporal_motion, fovpt_post) wrote;
 *                            FOVPT_E_NO_FRAME when there is none (no step yet, or fovpt_temporal_reset / fovpt_resize /
 *                            fovpt_set_scene since).  The next temporal step leaves it alone and overwrites the other set.
 *   fovpt_warp_motion        fovpt_warp in which the meshes that moved go on moving.  fovpt_warp re-aims the
 *                            static world; every skinned, morphed, rigged or rigidly moving mesh stays where it was at render time.
 *                            This call is fovpt_warp, operation for operation -- inputs and outputs, the context's warp buffers and
 *                            keys, fovpt_warp_counts, the stream and the ordering, images, fill_radius, the map and the classes, the
 *                            validation and the resolve -- with one difference: a source pixel that hits a mesh moved in the last
 *                            interval scatters an extrapolated point X* instead of X_s.  The last interval is the one ended by the
 *                            context's last temporal step (fovpt_temporal, fovpt_temporal_motion or fovpt_post, whichever ran
 *                            last).  With (u, v) the pixel's hit record and a', b', c' the positions its triangle's vertices had
 *                            when the step before the last one ran (fovpt_temporal_motion's quantities), every *, +, - one unfused
 *                            binary32 operation per component (tests/warp_motion_ref.py):
 *                              w0 = (1 - u) - v          X' = (w0 a' + u b') + v c'
 *                              d  = X_s - X'             X* = X_s + advance * d
 *                              v  = X* - eye_to          then fovpt_warp's a_k, px, py, fx, fy, landing test, depth word and key
 *                            X_s is the G-buffer position as stored.  A non-finite X* lands nowhere.  Hits on meshes that did not
 *                            move in that interval, every miss, every pixel when no mesh moved or advance is 0 (the call then
 *                            launches fovpt_warp's own scatter kernel), and every pixel when the last step knew nothing of the
 *                            motion (an update ran while the tracking of previous positions was still off: the first
 *                            fovpt_temporal_motion of a scene) are fovpt_warp's, bit for bit.  advance: how far past the rendered
 *                            frame the image is shown, in units of the interval between the last two temporal steps.
 *                            The hit records are not part of fovpt_gbuffer_ptrs: they are the context's, written by its last
 *                            G-buffer trace, whichever call made it.  gbuffer NULL: the call traces, as fovpt_warp does.  Non-NULL:
 *                            the pointers are used as fovpt_warp uses them, and the call checks on the host (one counter, stamped
 *                            at every trace; no device work) that the context's last trace was of the rendered frame's size and
 *                            camera and is newer than the last fovpt_render, geometry update, fovpt_resize and fovpt_set_scene.
 *                            With fovpt_temporal_gbuffer's set the loop update -> render -> post(MOTION) -> expose ->
 *                            temporal_gbuffer -> warp_motion -> update ... traces one G-buffer per frame.
 *                            All or nothing.  Everything fovpt_warp returns for the same arguments; FOVPT_E_INVALID: advance NaN,
 *                            infinite, below 0 or above FOVPT_WARP_MAX_ADVANCE, a non-zero reserved field; FOVPT_E_NO_FRAME: no
 *                            temporal step since create / fovpt_temporal_reset / fovpt_resize / fovpt_set_scene; tracking of
 *                            previous positions off (no fovpt_temporal_motion and no fovpt_post with MOTION on this scene yet); a
 *                            geometry update issued since the last temporal step (the previous positions and the step's G-buffer
 *                            no longer describe one frame); with a caller's gbuffer, the stamp check above.
 *   fovpt_warp_motion_defaults   host only, no context: both images, fill_radius 2, advance 1 (conventions, not measurements).
 * Out of scope.  Moving meshes in fovpt_warp itself: it warps them as if static; fovpt_warp_motion extrapolates them by one
 * interval's difference (no acceleration, and not their reflections and shadows).  Its resolve is fovpt_warp's: a strip that a mesh
 * vacates, if it is wider than fill_radius rings, stays class empty and keeps showing the source pixel -- the mesh's old image (on the
 * wall scene of tests/test_warp_motion_cpu.py already at advance 1 with a move of 8 px).  Resampling: a pixel is copied, not interpolated.  Packets: a packet's texel ownership belongs to the rendered camera, so
 * the warp is the last stage on the server, or a client's job after decoding: fovpt_packet_encode_depth sends the depth and the
 * camera along, fovpt_packet_decode_depth and fovpt_warp_depth are the client's calls (below, "depth packets").
 * On an MI355X at 1920 x 1080, both images, fill_radius 2, a call takes 0.050 .. 0.054 ms with a caller's G-buffer and 0.262 .. 0.265 ms with
 * its own trace over a slide, a turn and a dolly-in (fovpt_expose FIXED, a plain full-frame pass: 0.020 ms; one fovpt_render: 0.70 ms)
 * (DESIGN.md, section 21).  fovpt_warp_motion, same frame, a slide, advance 1, alternated with fovpt_warp in one process: 0.050 ms with
 * nothing moved (fovpt_warp's launches); 0.060 ms with a quarter of the meshes turning (62 % of the source pixels on moved meshes) and
 * 0.063 ms with all of them, against fovpt_warp's 0.050 ms, with the step's G-buffer; 0.279 and 0.284 ms against 0.267 and 0.269 ms
 * with its own trace; direct / filled / empty 92.2 / 3.4 / 4.4 % against fovpt_warp's 94.2 / 1.5 / 4.4 %.     */
typedef struct fovpt_warp_camera { fovpt_float3 eye, U, V, W; } fovpt_warp_camera;        /* 48 bytes: LaunchParams.camera's layout */
#define FOVPT_WARP_COLOR 1          /* warp the float4 image   */
#define FOVPT_WARP_RGBA  2          /* warp the rgba8 image    */
#define FOVPT_WARP_MAX_RADIUS 4
typedef struct fovpt_warp_config {  /* 32 bytes */
    int32_t images;                 /* FOVPT_WARP_* bits, at least one; default 3 */
    int32_t fill_radius;            /* 0 .. FOVPT_WARP_MAX_RADIUS; default 2 (a convention, not a measurement) */
    int32_t _reserved[6];           /* 0 */
} fovpt_warp_config;
struct fovpt_warp_counts {          /* 32 bytes, of the last fovpt_warp */
    uint64_t splatted;              /* source pixels that landed inside the frame */
    uint64_t direct, filled, empty; /* destination pixels by class; they sum to width * height */
};
int fovpt_warp_defaults(fovpt_warp_config* out);
int fovpt_warp(fovpt_ctx* ctx, const fovpt_launch_params* lp, const fovpt_warp_camera* to, const fovpt_warp_config* wc,
               const fovpt_gbuffer_ptrs* gbuffer /* NULL: traced by the call */, const fovpt_float4* in_color /* NULL: accum_buffer */,
               const uint32_t* in_rgba /* NULL: frame_buffer */, fovpt_float4* out_color, uint32_t* out_rgba /* NULL: the context's own */,
               uint32_t* out_map /* may be NULL */);
int fovpt_warp_buffers(fovpt_ctx* ctx, fovpt_float4** color, uint32_t** rgba);
int fovpt_warp_counts(fovpt_ctx* ctx, struct fovpt_warp_counts* out);
#define FOVPT_WARP_MAX_ADVANCE 4.0f
typedef struct fovpt_warp_motion_config {   /* 32 bytes */
    int32_t images;                 /* FOVPT_WARP_* bits, at least one; default 3 */
    int32_t fill_radius;            /* 0 .. FOVPT_WARP_MAX_RADIUS; default 2 */
    float   advance;                /* 0 .. FOVPT_WARP_MAX_ADVANCE, finite; default 1.0f: how far past the rendered frame the image is
                                       shown, in units of the interval between the last two temporal steps (a convention, not a
                                       measurement) */
    int32_t _reserved[5];           /* 0 */
} fovpt_warp_motion_config;
int fovpt_warp_motion_defaults(fovpt_warp_motion_config* out);
int fovpt_warp_motion(fovpt_ctx* ctx, const fovpt_launch_params* lp, const fovpt_warp_camera* to, const fovpt_warp_motion_config* mc,
                      const fovpt_gbuffer_ptrs* gbuffer /* NULL: traced by the call */, const fovpt_float4* in_color /* NULL: accum_buffer */,
                      const uint32_t* in_rgba /* NULL: frame_buffer */, fovpt_float4* out_color, uint32_t* out_rgba /* NULL: the context's own */,
                      uint32_t* out_map /* may be NULL */);
int fovpt_temporal_gbuffer(fovpt_ctx* ctx, fovpt_gbuffer_ptrs* out);

/* ---- gaze-metered focus distance and depth of field ----------------------------------------------------------------------------
 * New with this library.  Every other stage leaves the image sharp at all depths.  fovpt_focus meters the distance of what the eye
 * looks at from the G-buffer (meter -> adapt -> apply, the pattern of fovpt_expose: device state, no host synchronisation) and blurs
 * the frame by a per-pixel radius around that distance; fovpt_focus_state hands the metered distance to a varifocal or
 * vergence-aware client.  The stage is meant behind fovpt_post and ahead of fovpt_expose.
 *   fovpt_focus              works on the frame last issued with fovpt_render(ctx, lp) as it was rendered: its size, camera and
 *                            gaze.  gbuffer NULL: the call traces the rendered camera's G-buffer into fovpt_gbuffer's buffers (so it
 *                            needs the scene); non-NULL: the pointers are used as given, only prim and position are read, and the
 *                            caller vouches that they belong to the frame (fovpt_temporal_gbuffer's set saves the trace).
 *                            in_color NULL = accum_buffer; out_color / out_rgba NULL = the context's own (fovpt_focus_buffers:
 *                            allocated on first use together with an 8-byte-per-pixel scratch, reallocated by fovpt_resize, freed by
 *                            fovpt_destroy; a context that never calls the stage pays nothing); out_coc (may be NULL): the blur
 *                            radius per pixel, float.  Enqueued on fovpt_stream(), not synchronised, ordered like fovpt_denoise.
 *                            The definition, operation by operation (tests/focus_ref.py), every fp32 +, -, * and / one unfused
 *                            operation; w, h the frame size, a pixel is a hit iff prim != 0xffffffff, t = position.w,
 *                            min(a, b) = a < b ? a : b:
 *                              1 meter (AUTO)  cx, cy the rendered gaze (frame.c, unsigned 32 bits) as signed 64-bit integers.  A
 *                                          pixel (x, y) of the frame counts iff (x-cx)^2 + (y-cy)^2 <= meter_radius^2 in integers,
 *                                          it is a hit and t > 0 (in float).  With u the bits of t, bin = clamp((u >> 20) - 888,
 *                                          0, 255): fovpt_expose's bins, 8 per octave over 2^-16 .. 2^16.  h[bin] += 1, T = sum h.
 *                                          T == 0: focus_metered = the present focus, on a first step focus_default.  Otherwise
 *                                          k = min(T * rank_permille / 1000, T - 1) (integer division), b the smallest bin with
 *                                          h[0] + .. + h[b] > k, focus_metered the float with the bits ((b + 888) << 20) | 0x80000
 *                              2 adapt     in reciprocal distance.  D_m = 1.0f / focus_metered.  First step after create / reset:
 *                                          D = D_m; otherwise D = D + a * (D_m - D), a = adapt_nearer if D_m > D else adapt_farther;
 *                                          a later step with T == 0 leaves D as it is (D_m = D).  focus = 1.0f / D.  The state
 *                                          record gets focus_metered, inv_focus = D, focus, count = T, steps + 1.
 *                                          FOCUS_FIXED: D = 1.0f / focus_distance; nothing is metered, the state is untouched
 *                              3 radius    per pixel: i = 1.0f / t for a hit, 0.0f for a miss; s = strength * fabsf(i - D);
 *                                          r = s < (float)max_radius ? s : (float)max_radius; out_coc[p] = r
 *                              4 gather    per pixel p = (x, y): tp = t for a hit, +inf for a miss.  The taps q = (x + dx, y + dy),
 *                                          dy = -max_radius .. max_radius the outer loop, dx likewise the inner one; taps outside
 *                                          the frame are skipped.  re = (tq > tp) ? min(rq, rp) : rq -- a surface behind p does
 *                                          not bleed over p further than p itself is blurred, a surface in front spreads by its
 *                                          own radius --, e = re + 0.5f; the tap covers iff (float)(dx*dx + dy*dy) <= e * e.
 *                                          Only covering taps are added, in visiting order, into one running sum each:
 *                                          g = 1.0f / (e * e), den += g, num.c += g * in.c for c = r, g, b.  The centre always
 *                                          covers.  If it is the only covering tap out_color[p] = in_color[p], all four components
 *                                          bit for bit; otherwise (num.r / den, num.g / den, num.b / den, in_color[p].w).
 *                                          out_rgba[p] = make_color(reinhard(out_color[p].rgb * 16, 1)) as in every other stage.
 *                                          Outputs for non-finite or negative input colours, or for a caller's G-buffer with
 *                                          non-finite t, are unspecified.
 *                            So strength = 0, max_radius = 0 or a scene entirely at the focus distance returns the input bit for
 *                            bit, and an in-focus object keeps its pixels exactly, whatever lies behind it.
 *                            The state survives fovpt_resize and fovpt_set_probe; fovpt_focus_reset and fovpt_set_scene reset it.
 *                            All or nothing, checked before anything is enqueued.  FOVPT_E_INVALID: null ctx / lp / fc; an unknown
 *                            mode; meter_radius outside 0 .. FOVPT_FOCUS_MAX_METER_RADIUS; rank_permille outside 0 .. 1000;
 *                            max_radius outside 0 .. FOVPT_FOCUS_MAX_RADIUS; strength NaN, negative or above FOVPT_SIGMA_MAX;
 *                            focus_distance or focus_default outside [FOVPT_SIGMA_MIN, FOVPT_SIGMA_MAX] or NaN; an adapt rate
 *                            outside (0, 1] or NaN; non-zero reserved fields; a gbuffer whose size is not the frame's or with a
 *                            null prim or position; a null input; width * height >= 2^31; any output equal to an input (the colour,
 *                            the G-buffer's prim or position, the scratch: the kernels gather across pixels; base addresses are
 *                            compared) or to another output; a frame rendered with world > 1.  FOVPT_E_NO_FRAME,
 *                            FOVPT_E_NO_SCENE: as fovpt_warp (the scene only where the call traces).
 *   fovpt_focus_defaults     host only, no context.  CONVENTIONS, NOT MEASUREMENTS: AUTO, meter_radius 12, rank_permille 250 (the
 *                            nearer quartile: the eye settles on the nearer surface under the gaze), max_radius 6, strength 8,
 *                            focus_distance 1, focus_default 1, both adapt rates 1 (the caller derives 1 - exp(-dt / tau) from its
 *                            own frame time).  A thin lens of radius a in scene units has strength a * (h / 2) * |W| / |V|.
 *   fovpt_focus_buffers      addresses of the context's own focused outputs (allocated for the last frame if not yet).
 *   fovpt_focus_state        synchronises fovpt_stream() and copies the state record out; zeros before any AUTO step.  The struct
 *                            and the function share their name, so the struct has no typedef: write `struct fovpt_focus_state`.
 *   fovpt_focus_reset        the next AUTO step is a first step.  Enqueued on fovpt_stream().
 * Out of scope.  Bokeh shapes; partial occlusion (what a blurred foreground hides stays hidden); per-level radii; the periphery's
 * block copies are blurred as the pixels they are.
 * On an MI355X at 1920 x 1080 with a caller's G-buffer a call takes 0.049 ms where every tile is a copy (strength 0; 2.6 times
 * fovpt_expose FIXED, a plain full-frame pass: 0.019 ms), 0.153 ms with the defaults' cap of 6 on the atrium (mean radius 3.9 pixels;
 * with its own trace 0.355 ms) and 0.306 ms with every pixel at max_radius 8, the worst case (one fovpt_render of that frame:
 * 0.516 ms); the AUTO meter alone 0.004 ms at meter_radius 12 and 0.017 ms at 64.                        */
#define FOVPT_FOCUS_FIXED 0          /* focus at cfg.focus_distance; nothing is metered, the state is untouched */
#define FOVPT_FOCUS_AUTO  1
#define FOVPT_FOCUS_MAX_RADIUS 8         /* blur radius cap, pixels */
#define FOVPT_FOCUS_MAX_METER_RADIUS 64  /* gaze disc, pixels */
#define FOVPT_FOCUS_BINS 256
typedef struct fovpt_focus_config {  /* 64 bytes */
    int32_t mode, meter_radius, rank_permille, max_radius;
    float strength;            /* pixels of blur radius per unit of |1/t - 1/focus| (scene units); 0 = off */
    float focus_distance;      /* FIXED */
    float focus_default;       /* AUTO, first step with nothing to meter */
    float adapt_nearer, adapt_farther;   /* share of the way per step, in 1/distance, (0, 1] */
    int32_t _reserved[7];
} fovpt_focus_config;
struct fovpt_focus_state {     /* 32 bytes */
    float focus_metered, inv_focus, focus, _pad;
    uint64_t count;            /* T of the last metered step */
    uint64_t steps;            /* AUTO steps since create / reset */
};
int fovpt_focus_defaults(fovpt_focus_config* out);
int fovpt_focus(fovpt_ctx* ctx, const fovpt_launch_params* lp, const fovpt_focus_config* fc,
                const fovpt_gbuffer_ptrs* gbuffer /* NULL: traced by the call */, const fovpt_float4* in_color /* NULL: accum_buffer */,
                fovpt_float4* out_color, uint32_t* out_rgba /* NULL: the context's own */, float* out_coc /* may be NULL */);
int fovpt_focus_buffers(fovpt_ctx* ctx, fovpt_float4** color, uint32_t** rgba);
int fovpt_focus_state(fovpt_ctx* ctx, struct fovpt_focus_state* out);   /* synchronises fovpt_stream() */
int fovpt_focus_reset(fovpt_ctx* ctx);                                  /* enqueued */

/* ---- head-mounted display lens pre-distortion with chromatic correction ---------------------------------------------------------
 * New with this library.  fovpt_warp is a compositor's timewarp; its other half is the pre-distortion that cancels the headset's
 * lens, one radial polynomial per colour channel so that the lens's chromatic aberration cancels too.  fovpt_lens is that pass, for
 * a caller that drives a panel directly: an inverse-mapped resampling stage.  For every display pixel it computes where, per channel,
 * the rendered image is to be read, optionally re-aims that ray by a rotation-only late camera ("rotate and distort in one
 * gather"), and filters with nearest, bilinear or Catmull-Rom taps.  The stage is the last one ahead of the display (or of
 * fovpt_packet_*): render -> fovpt_post -> fovpt_focus -> fovpt_expose -> fovpt_lens.
 *   fovpt_lens               works on the frame last issued with fovpt_render(ctx, lp): its size and, only with `to`, its camera.
 *                            It needs no scene.  in_color NULL = accum_buffer; out_color / out_rgba NULL = the context's own
 *                            (fovpt_lens_buffers: allocated on first use, reallocated by fovpt_resize, freed by fovpt_destroy; a
 *                            context that never calls the stage pays nothing).  Enqueued on fovpt_stream(), not synchronised,
 *                            ordered like fovpt_denoise.
 *                            The definition, operation by operation (tests/lens_ref.py), every fp32 +, -, * and / one unfused
 *                            operation; w, h the frame size, (x, y) a destination pixel:
 *                              1  nx = (float)(2x + 1) / (float)w - 1.0f, ny likewise with h
 *                              2  px = (nx - center.x) * scale.x, py likewise; r2 = px * px + py * py
 *                              3  if !(r2 <= clip_r2) the pixel is outside the lens: out_color = border, all four components
 *                                 (NaNs fall here)
 *                              4  f = k0 + r2 * (k1 + r2 * (k2 + r2 * k3)).  Per channel c: fc = f * chroma[c],
 *                                 sx = (px * fc) * src_scale.x + src_center.x, sy likewise
 *                              5  only with `to`: a_k = (H[k][0] * sx + H[k][1] * sy) + H[k][2] for k = 0, 1, 2; the channel is
 *                                 valid iff a.z > 0; then sx = a.x / a.z, sy = a.y / a.z.  H = M [U_to V_to W_to], computed on the
 *                                 host in binary64 and rounded to fp32: M the rows of inverse(U V W) of the rendered camera (each
 *                                 entry rounded to fp32, as fovpt_warp and fovpt_temporal compute them), each entry of the product
 *                                 (m0 * b0 + m1 * b1) + m2 * b2.  to.eye is ignored: the re-aim is rotational (translation needs
 *                                 depth: that is fovpt_warp, ahead of this stage)
 *                              6  fx = ((sx + 1.0f) * 0.5f) * (float)w - 0.5f, fy likewise with h (fovpt_warp's pixel convention)
 *                              7  an invalid channel has the value border[c] exactly and reads no tap.  A channel is invalid if
 *                                 step 5 said so, or if !(fx >= -2.0f && fx <= (float)w + 1.0f), or the same for fy and h
 *                              8  otherwise the filter; a tap outside the frame reads border[c], and a window with no tap inside
 *                                 the frame gives border[c] exactly (the sums below would round).
 *                                 NEAREST   the tap (floor(fx + 0.5f), floor(fy + 0.5f))
 *                                 BILINEAR  x0 = floor(fx), tx = fx - x0, likewise in y; taps a = (x0, y0), b = (x0 + 1, y0) and
 *                                           the row below: top = (1.0f - tx) * a + tx * b, bottom likewise,
 *                                           v = (1.0f - ty) * top + ty * bottom
 *                                 BICUBIC   taps x0 - 1 .. x0 + 2, weights of t = tx (and of ty for the rows)
 *                                           w0 = ((-0.5f * t + 1.0f) * t - 0.5f) * t,  w1 = ((1.5f * t - 2.5f) * t) * t + 1.0f,
 *                                           w2 = ((-1.5f * t + 2.0f) * t + 0.5f) * t,  w3 = ((0.5f * t - 0.5f) * t) * t;
 *                                           a row is ((w0 * a0 + w1 * a1) + w2 * a2) + w3 * a3, the four rows y0 - 1 .. y0 + 2
 *                                           are combined the same way with the y weights; then v = v < 0.0f ? 0.0f : v
 *                              9  out_color = (v_r, v_g, v_b, 1.0f); out_rgba by `encode`, of out_color's rgb (a pixel outside
 *                                 the lens: of the border's), with make_color and reinhard of the resolve.  Outputs for non-finite
 *                                 input colours are unspecified
 *                            When the three chroma entries have equal bits the channels share one position, and the kernel does
 *                            one lookup in place of three: the same results by construction.
 *                            All or nothing, checked before anything is enqueued.  FOVPT_E_INVALID: null ctx / lp / lc; an unknown
 *                            filter or encode; non-zero reserved fields; a non-finite center, scale, k, chroma, src_center,
 *                            src_scale or border entry; a clip_r2 that is NaN or <= 0 (+inf is allowed); with `to`, a non-finite
 *                            entry of `to`, or a rendered camera whose [U V W] has a determinant of 0 or a non-finite one; a null
 *                            input; an output equal to the input or to the other output (the kernel gathers across pixels; base
 *                            addresses are compared); width * height >= 2^31; a frame rendered with world > 1.
 *                            FOVPT_E_NO_FRAME: as fovpt_focus.
 *   fovpt_lens_defaults      host only, no context.  CONVENTIONS, NOT MEASUREMENTS: BILINEAR, ENCODE_DISPLAY, center 0, both
 *                            scales (1, 1), src_center 0, clip_r2 +inf, border (0, 0, 0, 1), k = (1, 0.22, 0.24, 0) and
 *                            chroma = (0.996, 1, 1.014): the publicly documented coefficients of a first-generation
 *                            development-kit lens.  The defaults know no frame size: a caller sets scale.y = h / w and
 *                            src_scale.y = w / h (the lens is round, the NDC square is not) and divides both src_scale entries by
 *                            f(1), so that the mid-point of the left and right edges maps to itself (lens_for_frame of the Python
 *                            binding, lensForFrame of SimplePathtracer.h).
 *   fovpt_lens_buffers       addresses of the context's own outputs (allocated for the last frame if not yet).
 * Out of scope.  Mesh-based or look-up-table distortion; positional re-aim (fovpt_warp); resampling the rgba8 image; vignetting
 * compensation; distortion of packets on a client.
 * On an MI355X at 1920 x 1080 a call takes, as a multiple of fovpt_expose FIXED (a plain full-frame pass: 0.020 ms) measured beside it:
 * NEAREST 1.19 (equal chroma: one lookup) / 1.34 (distinct chroma: three), BILINEAR 1.46 / 1.76 (0.030 / 0.036 ms), BICUBIC 1.85 /
 * 3.86 (0.038 / 0.078 ms), BILINEAR with distinct chroma and a re-aim 1.89 (one fovpt_render of that frame: 0.655 ms) (DESIGN.md,
 * section 25).                                                                                                                     */
#define FOVPT_LENS_NEAREST  0
#define FOVPT_LENS_BILINEAR 1
#define FOVPT_LENS_BICUBIC  2          /* Catmull-Rom, 4 x 4 taps */
#define FOVPT_LENS_ENCODE_DISPLAY 0    /* out_rgba = make_color(o): the input is display-referred (fovpt_expose's colour) */
#define FOVPT_LENS_ENCODE_RESOLVE 1    /* out_rgba = make_color(reinhard(o * 16, 1)) as every other stage */
typedef struct fovpt_lens_config {     /* 128 bytes */
    int32_t filter, encode, _reserved0[2];
    float center[2];       /* lens axis in destination NDC */
    float scale[2];        /* destination NDC -> lens radius units */
    float k[4];            /* f = k0 + r2 * (k1 + r2 * (k2 + r2 * k3)) */
    float chroma[3];       /* per-channel factor on f: red, green, blue */
    float clip_r2;         /* r2 above it is outside the lens; +inf = none */
    float src_center[2], src_scale[2];   /* lens units -> source NDC */
    float border[4];       /* what lies outside the source image or the lens */
    int32_t _reserved[8];
} fovpt_lens_config;
int fovpt_lens_defaults(fovpt_lens_config* out);          /* host only, no context */
int fovpt_lens(fovpt_ctx* ctx, const fovpt_launch_params* lp, const fovpt_lens_config* lc,
               const fovpt_warp_camera* to /* NULL: no re-aim */, const fovpt_float4* in_color /* NULL: accum_buffer */,
               fovpt_float4* out_color, uint32_t* out_rgba /* NULL: the context's own */);
int fovpt_lens_buffers(fovpt_ctx* ctx, fovpt_float4** color, uint32_t** rgba);

/* ---- luminance moment history and variance-guided a-trous filter ------------------------------------------------------------------
 * New with this library.  fovpt_denoise's colour edge-stop is a guess that knows nothing of how noisy a pixel is, and the temporal
 * step carries no second moment.  This stage closes that gap the way SVGF does (Schied et al. 2017): fovpt_variance keeps temporally
 * reprojected first and second luminance moments per pixel (a spatial estimate where the history is short) and writes a variance
 * image; fovpt_variance_filter is an a-trous filter over a per-pixel G-buffer whose luminance edge-stop is scaled by that variance,
 * which it pushes through its iterations.  Neither reads the frame's guides, so both run on fovpt_reconstruct's or fovpt_post's
 * per-pixel output.  The loop they are meant for, tracing one G-buffer per frame:
 *   render -> fovpt_post(RECONSTRUCT | TEMPORAL | MOTION, out_motion) -> fovpt_temporal_gbuffer
 *          -> fovpt_variance(in_sample = accum_buffer, motion) -> fovpt_variance_filter(in_color = post's colour) -> focus / expose / lens
 * Both calls work on the frame last issued with fovpt_render(ctx, lp): its size, its passes and its camera.  Both are enqueued on
 * fovpt_stream(), not synchronised, ordered like fovpt_denoise, and all or nothing: every argument is checked before anything is
 * enqueued or any state moves.  Both are defined operation by operation (tests/variance_ref.py): every fp32 +, -, * and / one unfused
 * operation, beyond those only floor, min, max and comparisons -- no transcendental function, no square root.  w, h the frame size,
 * (x, y) a pixel, idx = y * w + x; lum(c) = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; sq3(a) = (a.x * a.x + a.y * a.y) + a.z * a.z,
 * dot likewise; edge(d) = max(0, 1 - d)^2; a pixel's fill is that of its last writer among the frame's passes, 1 where no pass writes.
 *   fovpt_variance           the moment step (one kernel).  gbuffer NULL = the rendered frame's G-buffer is traced by the call, as
 *                            fovpt_warp does (into fovpt_gbuffer's buffers; needs the scene); of a caller's G-buffer only position and
 *                            normal are read, never prim.  in_sample NULL = accum_buffer; motion NULL = the history is read at the
 *                            pixel itself; out_variance NULL = the context's own image.  The context owns two moment histories, used in
 *                            turn like the temporal step's, and the variance image, float4 per pixel each (allocated on first use,
 *                            reallocated by fovpt_resize, freed by fovpt_destroy; a context that never calls the stage pays nothing).
 *                            M: the rows of inverse(U V W) of the rendered camera as fovpt_lens step 5 takes them (binary64, each
 *                            entry rounded to fp32).
 *                              1  l = lum(in_sample[idx]), l2 = l * l
 *                              2  the pixel is a miss iff gbuffer.position[idx].w < 0.  A hit: v = X - eye,
 *                                 z_p = (M[2].x * v.x + M[2].y * v.y) + M[2].z * v.z; a miss: z_p = -1
 *                              3  mv = motion ? motion[idx] : (0, 0, z_p, 1); no history if mv.w == 0; px = (float)x + mv.x, py
 *                                 likewise, zr = mv.z; no history unless px >= -1 && px < w && py >= -1 && py < h (a NaN fails)
 *                              4  x0 = floor(px), fx = px - x0, likewise in y; the taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1),
 *                                 (x0 + 1, y0 + 1) with weights (1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy.  A tap q
 *                                 inside the frame is kept iff the previous record's (z_q < 0) equals the pixel's miss class and, for
 *                                 hits, fabsf(z_q - zr) <= depth_tolerance * zr.  sw = sum of the kept weights in tap order; if
 *                                 sw >= 1 / 64: m1 = (sum M1_q * w) / sw, m2 and n_h likewise; otherwise n_h = 0.  The first step,
 *                                 and the first after fovpt_variance_reset, fovpt_resize or fovpt_set_scene, has no history anywhere
 *                              5  n = min(n_h + 1, (float)history_cap).  n == 1: M1 = l, M2 = l2 bit for bit; otherwise
 *                                 M1 = m1 + (1 / n) * (l - m1), M2 = m2 + (1 / n) * (l2 - m2).  The new record is (M1, M2, n, z_p)
 *                              6  n >= (float)spatial_below: mean = M1, var = max(0, M2 - M1 * M1).  Otherwise the spatial estimate
 *                                 over the current frame: taps q = clamp(p + fill * (i, j)), i, j in -R .. R (rows outer),
 *                                 R = spatial_radius; the centre has weight 1, another tap weight 1 iff its class equals the pixel's
 *                                 and, for hits, sq3(N_q - N_p) <= normal_tolerance and fabsf(dot(N_p, X_q - X_p)) <=
 *                                 depth_tolerance * t_p, else 0.  s0 = sum w, s1 = sum w * l_q, s2 = sum w * (l_q * l_q);
 *                                 mean = s1 / s0, var = max(0, s2 / s0 - mean * mean).  (Stepping by the fill: a block-filled pixel
 *                                 never counts its own copies)
 *                              7  out_variance[idx] = (rel, var, mean, n), rel = var / (mean * mean + 1e-8f): the squared coefficient
 *                                 of variation, the same for a colour and for that colour divided by its albedo
 *                            FOVPT_E_INVALID: null ctx / lp / vc; a value out of range (NaN included); non-zero reserved fields; a
 *                            G-buffer of another size or with a null position or normal; an output that is an input or a history
 *                            (base addresses are compared); a rendered camera whose [U V W] is singular; width * height >= 2^31; a
 *                            frame rendered with world > 1.  FOVPT_E_NO_FRAME, FOVPT_E_NO_SCENE: as fovpt_reconstruct (the scene only
 *                            where the call traces).  Outputs for non-finite colours are unspecified.  fovpt_set_probe keeps the
 *                            history: a caller who changes the lighting resets.
 *   fovpt_variance_defaults  host only, no context.  CONVENTIONS, NOT MEASUREMENTS: history_cap 16, spatial_below 4 and
 *                            spatial_radius 3 (a 7 x 7 window) are SVGF's; the tolerances 0.02 and 0.1 are fovpt_temporal's.
 *   fovpt_variance_buffers   the context's own variance image and the moment history the last step wrote (allocated for the last
 *                            frame if not yet).
 *   fovpt_variance_reset     the next step has no history (takes effect in call order).
 *   fovpt_variance_filter    gbuffer NULL = traced by the call; position, normal and (with demodulate) albedo of a caller's are
 *                            read.  in_color NULL = accum_buffer; variance NULL = the context's own image as the last fovpt_variance
 *                            into it left it; out_color / out_rgba NULL = the context's own (fovpt_variance_filter_buffers).
 *                              prep   the level byte is fovpt_denoise's: iterations n by the fill of the last writer (0 where no pass
 *                                     writes), and log2(fill).  D = demodulate ? demod(albedo[idx]) : 1, demod the denoiser's;
 *                                     I = C / D; v0 = variance[idx].x * (lum(I) * lum(I)); J = (I, v0).  A pixel with n = 0 gets
 *                                     out_color = (C.rgb, 1) and its tone map here
 *                              iteration it = 0 .. max n - 1, for the pixels with it < n (the others keep J); s = fill * 2^it:
 *                                1  g = sum G_ij * J.w(clamp(p + fill * (i, j))), i, j in -1 .. 1 (rows outer),
 *                                   G = [1/16 1/8 1/16; 1/8 1/4 1/8; 1/16 1/8 1/16]
 *                                2  kl = 1 / ((luminance_sigma * luminance_sigma) * g + 1e-6f) (the scale is the same in every
 *                                   iteration: the variance shrinks instead)
 *                                3  25 taps q = clamp(p + s * (dx, dy)), dy outer, B3 weights H = (1/16, 1/4, 3/8, 1/4, 1/16):
 *                                   d = lum(I_q) - lum(I_p), wl = edge((d * d) * kl); a class mismatch: wn = wz = 0; both misses: 1;
 *                                   both hits: wn = edge(sq3(N_q - N_p) * inv_n), wz = edge(((dz * dz) * inv_z) / (t_p * t_p)),
 *                                   dz = dot(N_p, X_q - X_p) (fovpt_reconstruct's expression), inv_n = 1 / normal_sigma^2 and
 *                                   inv_z = 1 / depth_sigma^2 in fp32 on the host.  wt = (((H_dx * H_dy) * wl) * wn) * wz;
 *                                   sw += wt, acc += I_q * wt, sv += (wt * wt) * v_q
 *                                4  I' = acc / sw, v' = sv / (sw * sw) (the centre tap keeps sw >= 9 / 64)
 *                              output of a pixel with n >= 1: I * D with alpha 1, rgba8 = make_color(reinhard(out * 16, 1))
 *                            Errors as fovpt_variance's, with: an iteration count outside 0 .. FOVPT_DENOISE_MAX_ITERATIONS, a sigma
 *                            outside [FOVPT_SIGMA_MIN, FOVPT_SIGMA_MAX], demodulate neither 0 nor 1, a null albedo with demodulate,
 *                            an output equal to an input or to the other output (the kernels gather), and FOVPT_E_NO_FRAME when
 *                            variance is NULL and no fovpt_variance has written the context's image at this frame size.
 *   fovpt_variance_filter_defaults   host only.  CONVENTIONS, NOT MEASUREMENTS: iterations 0 / 2 / 4 / 4, luminance_sigma 4 (SVGF's),
 *                            normal_sigma 0.5 and depth_sigma 0.05 (fovpt_reconstruct's), demodulate 1.
 * What is SVGF here: the moment history with its length, the spatial fallback, the variance-scaled luminance stop, the 3 x 3 prefilter
 * and the variance carried through the iterations.  What is not: the colour history stays fovpt_temporal's (with its own length), and
 * the weights are this library's (squared-linear edge, plane distance), not exponentials.
 * Out of scope.  A FOVPT_POST_* bit for this stage; a neighbourhood clamp of the colour history; variance of reflections and shadows
 * under motion; resetting the moments when a pixel changes foveation level (the cap bounds it); world > 1.
 * On an MI355X at 1920 x 1080, on fovpt_post's G-buffer, a call takes: fovpt_variance 0.258 ms as a first step (the window everywhere)
 * and 0.034 ms in steady state, fovpt_variance_filter at its defaults 0.587 ms, measured beside fovpt_denoise at its defaults (0.341 ms:
 * ratios 0.76 / 0.10 / 1.72) and one fovpt_render (0.687 ms).  On the 384 x 216 quality path the filter behind fovpt_post takes the
 * periphery's RMSE from 0.0451 to 0.0386 and the middle ring's from 0.0433 to 0.0268; luminance_sigma 1 / 2 / 8 give 0.0390 / 0.0386 /
 * 0.0387 and 0.0317 / 0.0281 / 0.0264.                                                                       */
typedef struct fovpt_variance_config {            /* 32 bytes */
    int32_t history_cap;           /* 1 .. FOVPT_TEMPORAL_MAX_HISTORY; default 16                                          */
    int32_t spatial_below;         /* a history shorter than this takes the spatial estimate: 0 .. history_cap + 1; 4      */
    int32_t spatial_radius;        /* 1 .. 3; default 3                                                                    */
    float depth_tolerance;         /* 0 .. 1; default 0.02                                                                 */
    float normal_tolerance;        /* 0 .. 4; default 0.1                                                                  */
    int32_t _reserved[3];
} fovpt_variance_config;
typedef struct fovpt_variance_filter_config {     /* 48 bytes */
    int32_t iterations_fovea, iterations_middle, iterations_periphery, iterations_uniform;   /* 0 .. FOVPT_DENOISE_MAX_ITERATIONS; 0 / 2 / 4 / 4 */
    float luminance_sigma;         /* FOVPT_SIGMA_MIN .. MAX; default 4    */
    float normal_sigma;            /* default 0.5                          */
    float depth_sigma;             /* default 0.05                         */
    int32_t demodulate;            /* 0 / 1; default 1                     */
    int32_t _reserved[4];
} fovpt_variance_filter_config;
int fovpt_variance_defaults(fovpt_variance_config* out);          /* host only, no context */
int fovpt_variance(fovpt_ctx* ctx, const fovpt_launch_params* lp, const fovpt_variance_config* vc,
                   const fovpt_gbuffer_ptrs* gbuffer /* NULL: traced by the call */, const fovpt_float4* in_sample /* NULL: accum_buffer */,
                   const fovpt_float4* motion /* NULL: history read at the pixel itself */, fovpt_float4* out_variance /* NULL: the context's own */);
int fovpt_variance_buffers(fovpt_ctx* ctx, fovpt_float4** variance, const fovpt_float4** moments);
int fovpt_variance_reset(fovpt_ctx* ctx);
int fovpt_variance_filter_defaults(fovpt_variance_filter_config* out);   /* host only, no context */
int fovpt_variance_filter(fovpt_ctx* ctx, const fovpt_launch_params* lp, const fovpt_variance_filter_config* fc,
                          const fovpt_gbuffer_ptrs* gbuffer /* NULL: traced by the call */, const fovpt_float4* in_color /* NULL: accum_buffer */,
                          const fovpt_float4* variance /* NULL: the context's own */, fovpt_float4* out_color, uint32_t* out_rgba /* NULL: the context's own */);
int fovpt_variance_filter_buffers(fovpt_ctx* ctx, fovpt_float4** color, uint32_t** rgba);

/* ---- image quality of a foveated frame: per-level error, SSIM and eccentricity profile -------------------------------------------
 * New with this library.  Choosing radii, spp, denoiser iterations, history caps or BC1 for a level asks one question: how good is
 * the frame, and where in the visual field does its error sit?  fovpt_quality answers it on the device, in stream order, with no
 * host synchronisation: it compares two display-referred rgba8 images of the frame last rendered (a test image against a
 * reference: a converged render, the uncoded frame, ...) and leaves exact integer sums in a small device record.  Everything in it
 * is an integer, or one binary64 quotient of exact integers, so the result does not depend on grid, block or summation order.
 *   fovpt_quality            works on the frame last issued with fovpt_render(ctx, lp) as it was rendered (its passes, its gaze
 *                            frame.c and its FOV_OFF flag).  test_rgba NULL = lp->frame.frame_buffer; out_sums NULL = the context's
 *                            own record (fovpt_quality_read; made on first use, freed by fovpt_destroy); out_class: one byte per
 *                            pixel, or NULL.  test_rgba may be ref_rgba (all errors zero).  Enqueued on fovpt_stream(), not
 *                            synchronised, ordered like fovpt_denoise; with caller-provided out_sums records any number of
 *                            measurements may be in flight.  Writes out_sums (every byte), out_class if given and its own scratch,
 *                            nothing else.  The definition, operation by operation (tests/quality_ref.py), with R, G, B the low
 *                            three bytes of a pixel (alpha is ignored), T the test and F the reference image:
 *                              1 class       of pixel (x, y): UNWRITTEN where no pass of the frame writes the pixel; otherwise
 *                                            UNIFORM on a FOV_OFF frame; otherwise by the fill of the pixel's last writer (as
 *                                            fovpt_expose's METER_GAZE): 4 PERIPHERY, 2 MIDDLE, anything else FOVEA.
 *                                            out_class[y * w + x] = that class
 *                              2 error sums  per class k: pixels[k] += 1; sq_err[k][c] += (T_c - F_c)^2 for c = r, g, b;
 *                                            differing[k] += 1 if any channel differs; max_err[k] = max(max_err[k], max_c |T_c - F_c|)
 *                              3 profile     (QUALITY_PROFILE, else both arrays 0) dx = x - (int64)(int32)frame.c.x, dy likewise,
 *                                            d2 = dx^2 + dy^2, ring = min(63, isqrt(d2) / ring_width) with isqrt the floor integer
 *                                            square root; ring_pixels[ring] += 1, ring_sq_err[ring] += the three channels' squared
 *                                            differences.  Every pixel counts, whatever its class
 *                              4 SSIM        (QUALITY_SSIM, else windows and ssim_q20 0) luma Y = (54 R + 183 G + 19 B + 128) >> 8.
 *                                            Windows are 8 x 8 pixels with origins (4i, 4j), 4i + 8 <= w, 4j + 8 <= h (a frame
 *                                            narrower or lower than 8 has none).  With the integer sums sx, sy, sxx, syy, sxy of a
 *                                            window's test (x) and reference (y) luma and C1 = 26634, C2 = 239708 ((0.01 * 255)^2
 *                                            * 4096 and (0.03 * 255)^2 * 4096, rounded), in int64:
 *                                              A = 2 sx sy + C1, B = 2 (64 sxy - sx sy) + C2, C = sx^2 + sy^2 + C1,
 *                                              D = (64 sxx - sx^2) + (64 syy - sy^2) + C2, N = A B, M = C D (|N|, M < 2^57),
 *                                              q = (int64)rint(((double)N / (double)M) * 1048576.0)
 *                                            every operation one IEEE binary64 operation, the conversions round to nearest even.
 *                                            The window's class k is that of pixel (x0 + 4, y0 + 4): windows[k] += 1, ssim_q20[k] += q
 *                              5 header      width, height, ring_width, flags echo the call; _pad = 0
 *                            All or nothing, checked before anything is enqueued.  FOVPT_E_INVALID: null ctx / lp / cfg / ref_rgba;
 *                            unknown flag bits; ring_width outside 1 .. FOVPT_QUALITY_MAX_RING_WIDTH; non-zero reserved fields; a
 *                            frame rendered with world > 1 (a shard does not see the frame); width * height >= 2^31; test_rgba NULL
 *                            with a null frame_buffer.  FOVPT_E_NO_FRAME: nothing rendered since create / resize, or
 *                            lp->frame.size differs.
 *   fovpt_quality_defaults   host only, no context.  SSIM | PROFILE; ring_width 16 is A CONVENTION, NOT A MEASUREMENT.
 *   fovpt_quality_read       synchronises fovpt_stream() and copies the context's own record out (all zero before the first
 *                            fovpt_quality with out_sums NULL).
 *   fovpt_quality_host       the same definition on host images, host only, no context, no device (also in libfovpt_loader.so):
 *                            the classes are handed in (one byte per pixel, each below FOVPT_QUALITY_CLASSES; NULL: all UNIFORM),
 *                            and the gaze as two integers.  FOVPT_E_INVALID: null test / ref / cfg / out, w or h < 1,
 *                            w * h >= 2^31, a bad config, a class byte out of range.
 *   fovpt_quality_mse / _psnr / _ssim / _score   host only, binary64, of a record (cls -1: every class but UNWRITTEN):
 *                            mse = sum_c sq_err / (3 pixels); psnr = 10 log10(65025 / mse), +inf at mse 0; ssim = ssim_q20 /
 *                            (1048576 windows); score = sum_k w_k sum_c sq_err[k] / (3 sum_k w_k pixels[k]), a weighted mse over the
 *                            five classes.  NaN for an empty class (no pixels, no windows, no weight), a null record or a cls
 *                            outside -1 .. 4.
 * On an MI355X at 1920 x 1080 a call takes 0.054 ms with no flags, 0.061 ms with SSIM, 0.059 ms with PROFILE and 0.079 ms with both,
 * measured beside fovpt_expose AUTO / METER_GAZE (one writer search per pixel and a two-kernel reduction too: 0.063 ms), fovpt_expose
 * FIXED (0.021 ms) and one fovpt_render of that frame (0.633 ms): 0.86, 0.96, 0.94 and 1.26 times AUTO / GAZE. */
#define FOVPT_QUALITY_SSIM     1   /* also the SSIM sums            */
#define FOVPT_QUALITY_PROFILE  2   /* also the eccentricity profile */
#define FOVPT_QUALITY_CLASSES  5
#define FOVPT_QUALITY_FOVEA     0
#define FOVPT_QUALITY_MIDDLE    1
#define FOVPT_QUALITY_PERIPHERY 2
#define FOVPT_QUALITY_UNIFORM   3
#define FOVPT_QUALITY_UNWRITTEN 4
#define FOVPT_QUALITY_RINGS    64
#define FOVPT_QUALITY_MAX_RING_WIDTH 65536
typedef struct fovpt_quality_config {     /* 32 bytes */
    int32_t flags;                        /* FOVPT_QUALITY_SSIM | FOVPT_QUALITY_PROFILE */
    int32_t ring_width;                   /* pixels per ring of the profile, 1 .. FOVPT_QUALITY_MAX_RING_WIDTH */
    int32_t _reserved[6];
} fovpt_quality_config;
typedef struct fovpt_quality_sums {       /* 1344 bytes */
    uint64_t pixels[FOVPT_QUALITY_CLASSES], differing[FOVPT_QUALITY_CLASSES], sq_err[FOVPT_QUALITY_CLASSES][3];
    uint32_t max_err[FOVPT_QUALITY_CLASSES], _pad;
    uint64_t windows[FOVPT_QUALITY_CLASSES];
    int64_t ssim_q20[FOVPT_QUALITY_CLASSES];
    uint64_t ring_pixels[FOVPT_QUALITY_RINGS], ring_sq_err[FOVPT_QUALITY_RINGS];
    uint32_t width, height, ring_width, flags;
} fovpt_quality_sums;
int fovpt_quality_defaults(fovpt_quality_config* out);
int fovpt_quality(fovpt_ctx* ctx, const fovpt_launch_params* lp, const fovpt_quality_config* qc,
                  const uint32_t* test_rgba /* NULL: lp->frame.frame_buffer */, const uint32_t* ref_rgba,
                  fovpt_quality_sums* out_sums /* device; NULL: the context's own record */,
                  uint8_t* out_class /* device, one byte per pixel, or NULL */);
int fovpt_quality_read(fovpt_ctx* ctx, fovpt_quality_sums* out /* host */);
int fovpt_quality_host(const uint32_t* test, const uint32_t* ref, int w, int h, const uint8_t* classes /* NULL: all UNIFORM */,
                       int64_t gaze_x, int64_t gaze_y, const fovpt_quality_config* qc, fovpt_quality_sums* out);
double fovpt_quality_mse(const fovpt_quality_sums* s, int cls /* -1: all classes but UNWRITTEN */);
double fovpt_quality_psnr(const fovpt_quality_sums* s, int cls);
double fovpt_quality_ssim(const fovpt_quality_sums* s, int cls);
double fovpt_quality_score(const fovpt_quality_sums* s, const double weights[FOVPT_QUALITY_CLASSES]);

/* ---- foveated frame packets: a frame off the device, small and without stopping the renderer -----------------------------------
 * New with this library.  fovpt_download drains every stream and copies a whole frame into pageable memory.  A foveated frame
 * is described exactly by one value per launch index -- at the shipped radii 74 / 241 a 1920 x 1080 frame has 211 149 of them,
 * 845 KB against 8.3 MB -- and the library knows which launch index wrote each pixel last (the resolve's writer search).  A
 * packet is that description, self-contained: a 128-byte header and one rgba8 texel array per pass, little endian (the
 * definition in integers: tests/packet_ref.py).  It is the last stage behind fovpt_post / fovpt_expose.
 *   layout    fovpt_packet_header, then per pass (launch order: P, M, F; FOV_OFF: one) gw * gh texels, row-major ly * gw + lx,
 *             back to back (the first at byte 128).  The header's pass records are those of the frame as rendered; it carries no
 *             gaze and no radii, a decoder needs neither.
 *   encode    a launch index OWNS the pixels whose last writer it is.  A texel with n owned pixels: n == 0 -> 0x00000000, else
 *             each of r, g, b = (sum + n / 2) / n of the owned pixels' 8-bit codes (integer division), alpha 0xff.  On the raw
 *             frame every owned pixel is equal, so the texel is that pixel.
 *   NEAREST   a texel with alpha != 0 writes its value to its block, pixels min((l * factor + off + u) mod 2^32, dim - 1) for
 *             u < fill on both axes; texels write in pass order, within a pass in ascending (ly, lx); later writes win; pixels
 *             no texel reaches keep what the output held.  decode(encode(raw frame)) is the raw frame on every written pixel.
 *   SMOOTH    a pixel whose NEAREST texel (lx, ly) has fill == factor > 1 and whose block anchor (ix, iy) satisfies
 *             0 <= x - ix < fill and 0 <= y - iy < fill is regular: dx = 2 (x - ix) + 1 - fill, sx = dx > 0 ? 1 : -1, neighbour
 *             weight |dx|, own weight 2 fill - |dx|, the same along y; the taps (lx, ly), (lx + sx, ly), (lx, ly + sy),
 *             (lx + sx, ly + sy) of the same pass carry the products.  A tap counts inside the grid with alpha != 0 (the own one
 *             always does); each channel is (sum w c + W / 2) / W over the counted taps, alpha 0xff.  Every other pixel gets its
 *             NEAREST value.  Seams between passes stay as they are.
 *   fovpt_packet_describe    host only: the header fovpt_packet_encode would write (header.bytes sizes the caller's buffer).
 *   fovpt_packet_encode      works on the frame last issued with fovpt_render(ctx, lp) as it was rendered, like every post stage.
 *                            in_rgba: any device rgba8 image of the frame's size (the post, expose or denoise outputs), NULL =
 *                            frame_buffer.  out_packet: device memory, header.bytes large, 4-byte aligned; written whole -- header
 *                            and zero texels included -- and nothing else is.  Enqueued on fovpt_stream(), not synchronised,
 *                            ordered like fovpt_denoise.  One thread per texel, no atomics (k_packet_encode).
 *   fovpt_packet_submit      encodes into the device buffer of the next of FOVPT_PACKET_SLOTS slots (round robin; *slot tells
 *                            which) and copies it to the slot's pinned host buffer on a copy stream of the context's own, behind
 *                            an event.  Never waits for the GPU, except for the copy of the slot it is about to reuse if that is
 *                            still in flight.
 *   fovpt_packet_wait        waits for that slot's copy alone -- frames and stages issued later keep running -- and returns the
 *                            pinned host pointer, valid until the slot is submitted again (fovpt_resize and fovpt_set_scene leave
 *                            it readable; fovpt_destroy frees it).
 *   fovpt_packet_decode      device decoder (one thread per pixel, k_packet_decode): header on the host, packet and out_rgba
 *                            (header's width x height) on the device.  Enqueued on fovpt_stream().  Needs no rendered frame.
 *                            It searches each pixel's last texel the way the resolve searches its last writer, which asks that
 *                            (gw - 1) * factor and (gh - 1) * factor stay below 2^31 - 8 (any packet the encoder makes; the host
 *                            decoder takes every valid packet).
 *   fovpt_packet_check       no context, both libraries (libfovpt_loader.so too): FOVPT_OK if the bytes are a valid packet.
 *   fovpt_packet_decode_host no context, both libraries: the decoder for a client, plain C++.  out_rgba: width x height pixels,
 *                            which must be the packet's.  The two never read outside [packet, packet + bytes) nor write outside
 *                            the output.
 * All or nothing, checked before anything is enqueued.  encode / submit / describe: FOVPT_E_INVALID for a null ctx / lp / output,
 * a frame rendered with world > 1 (a shard does not see the frame) or one whose packet would not pass fovpt_packet_check (a side
 * above 16384, more than 2^26 launch indices); FOVPT_E_NO_FRAME: nothing rendered since create / resize, or lp->frame.size
 * differs, or a null frame_buffer with in_rgba NULL.  wait: FOVPT_E_INVALID for a slot out of range or never submitted.  check /
 * decode_host / decode: FOVPT_E_INVALID for a wrong magic or version; a bytes field above the bytes given or below 128; width /
 * height outside 1 .. 16384 or other than the output's; npass outside 1 .. 3; a non-zero reserved field or unused pass entry; gw
 * or gh 0; more than 2^26 texels in total; factor 0; fill outside 1 .. 8; a texel offset below 128 or not a multiple of 4;
 * offset + 4 gw gh above the bytes field (in 64 bits); a mode other than 0 / 1; null pointers.
 * A context that never calls these allocates nothing for them and creates no stream.
 * On an MI355X at 1920 x 1080, radii 148 / 482 (C3, two frames in flight): render + fovpt_packet_submit / _wait takes 0.831 ms
 * per frame, render + fovpt_download of the frame 0.988 ms, render alone 0.699 ms; 1 810 768 bytes reach the host per frame
 * instead of 8 294 400; k_packet_encode takes 0.039 ms, k_packet_decode 0.013 ms (NEAREST) / 0.021 ms (SMOOTH).  Against
 * fovpt_post's rgba8 output the decoded frame is exact in the fovea and 13 .. 17 codes RMSE off in the other levels with NEAREST,
 * 20 .. 27 with SMOOTH.                                                                                   */
#define FOVPT_PACKET_MAGIC   0x4b505646u   /* "FVPK" */
#define FOVPT_PACKET_VERSION 1
#define FOVPT_PACKET_SLOTS   4
#define FOVPT_PACKET_NEAREST 0
#define FOVPT_PACKET_SMOOTH  1
typedef struct fovpt_packet_pass {      /* 32 bytes */
    uint32_t gw, gh;                    /* the pass's launch grid: one texel per launch index, row-major, ly * gw + lx */
    uint32_t factor, fill;              /* pixel index of a launch = l * factor + off (uint32, wraps); block of fill x fill */
    uint32_t offx, offy;
    uint32_t texels;                    /* byte offset of the texel array from the start of the packet, multiple of 4 */
    uint32_t _reserved;                 /* 0 */
} fovpt_packet_pass;
typedef struct fovpt_packet_header {    /* 128 bytes */
    uint32_t magic, version, bytes, sequence;   /* bytes: the whole packet; sequence: the caller's, copied through */
    int32_t width, height;
    uint32_t npass, _reserved;          /* 1 .. 3 passes in launch order (P, M, F; FOV_OFF: one) */
    fovpt_packet_pass pass[3];          /* unused entries all zero */
} fovpt_packet_header;
int fovpt_packet_describe(fovpt_ctx* ctx, const fovpt_launch_params* lp, uint32_t sequence, fovpt_packet_header* out);
int fovpt_packet_encode(fovpt_ctx* ctx, const fovpt_launch_params* lp, const uint32_t* in_rgba /* NULL = frame_buffer */,
                        uint32_t sequence, void* out_packet /* device, header.bytes large */);
int fovpt_packet_submit(fovpt_ctx* ctx, const fovpt_launch_params* lp, const uint32_t* in_rgba, uint32_t sequence, int* slot);
int fovpt_packet_wait(fovpt_ctx* ctx, int slot, const void** packet, size_t* bytes);      /* pinned host memory */
int fovpt_packet_decode(fovpt_ctx* ctx, const fovpt_packet_header* header /* host */, const void* packet /* device */,
                        int mode, uint32_t* out_rgba /* device, header's width x height */);
int fovpt_packet_check(const void* packet, size_t bytes);
int fovpt_packet_decode_host(const void* packet, size_t bytes, int mode, uint32_t* out_rgba, int width, int height);

/* ---- coded frame packets: levels as BC1 blocks, encoded on the device -----------------------------------------------------------
 * New with this library (the definition in integers: tests/packet_bc_ref.py).  A coded packet has magic
 * "FVPC", version 1 and the header above; the eighth word of a pass record (_reserved in the struct) is the pass's codec:
 *   FOVPT_PACKET_RAW   4 * gw * gh bytes of texels, as in an "FVPK" packet
 *   FOVPT_PACKET_BC1   8 * ceil(gw / 4) * ceil(gh / 4) bytes: BC1 / DXT1 blocks, row-major by * ceil(gw / 4) + bx, block (bx, by)
 *                      over texels (4 bx .. 4 bx + 3, 4 by .. 4 by + 3); texels beyond the grid count as dead
 * The arrays lie back to back from byte 128 at multiples of 4.  The texels that get coded are those of fovpt_packet_encode.
 *   block     L: the block's texels with alpha != 0.  L empty: 00 00 00 00 ff ff ff ff.  Else per channel lo / hi = min / max over
 *             L; ref = the channel with the largest hi - lo (ties: g, r, b); endpoint A takes hi_ref, B lo_ref; another channel k
 *             gives A hi_k and B lo_k unless s_k = sum over L of (2 c_k - lo_k - hi_k)(2 c_ref - lo_ref - hi_ref) < 0, then A lo_k
 *             and B hi_k.  565: q5(c) = (31 c + 127) / 255, q6(c) = (63 c + 127) / 255, a = q5(A_r) << 11 | q6(A_g) << 5 | q5(A_b).
 *             a == b, or a dead texel in the block: color0 = min(a, b), color1 = max(a, b) -- the 3-colour mode, index 3
 *             transparent; else color0 = max, color1 = min (4 colours).  Palette from e5(v) = v << 3 | v >> 2, e6(v) = v << 2 |
 *             v >> 4: P2 = (2 P0 + P1 + 1) / 3, P3 = (P0 + 2 P1 + 1) / 3 (4 colours), P2 = (P0 + P1 + 1) / 2 (3 colours).  A live
 *             texel's index: the opaque entry with the least squared distance, ties to the lowest; a dead texel's: 3.  Bytes:
 *             color0, color1 (LE16), a 32-bit LE word with texel (x, y) at bits 2 (4 y + x).
 *   decode    index 3 with color0 <= color1: 0x00000000; else 0xff000000 | b << 16 | g << 8 | r of the palette entry.  Liveness
 *             survives texel by texel, so NEAREST writes exactly the pixels it writes for the raw packet.
 * expand(coded packet) -- every BC1 pass replaced by its decoded texels -- is a valid "FVPK" packet, and NEAREST / SMOOTH of a
 * coded packet are NEAREST / SMOOTH of that.  fovpt_packet_check, fovpt_packet_decode_host and fovpt_packet_decode take both
 * magics; for "FVPC" the rejections are those above with the pass word a codec in {0, 1} and the array's end computed from
 * the codec (in 64 bits).
 *   fovpt_packet_defaults        codec[] = FOVPT_PACKET_BY_FILL: a pass is BC1 if its fill at describe time is above 1, else raw
 *                                (the fovea, and the one pass of FOV_OFF, stay exact).
 *   fovpt_packet_describe_coded / _encode_coded / _submit_coded   as their raw counterparts -- ordering, checks, error codes, the
 *                                same four slots (raw and coded submits may alternate, fovpt_packet_wait serves both) --, with
 *                                cfg->codec[p] the codec of launch pass p: FOVPT_PACKET_RAW, _BC1 or _BY_FILL.  Additionally
 *                                FOVPT_E_INVALID for a null cfg, another codec, a non-zero entry beyond the frame's passes (other
 *                                than _BY_FILL) or a non-zero _reserved.  k_packet_encode_coded: 16 lanes per block.
 * At 1920 x 1080, radii 148 / 482: 537 752 bytes with P and M coded, 227 536 with all three, against 1 810 768.  On an MI355X
 * k_packet_encode_coded takes 0.042 ms (k_packet_encode: 0.039), the coded decoders 0.015 ms (NEAREST) / 0.031 ms (SMOOTH); the
 * frame loop with a coded submit per frame takes 0.817 ms against 0.812 ms with a raw one.  The block code is a range fit: on
 * fovpt_post's output of a 1 / 2 spp periphery the decoded coded levels are 15 .. 16 codes RMSE off the decoded raw packet, and a
 * coded fovea 17: keep the fovea raw.                                                                     */
#define FOVPT_PACKET_MAGIC_CODED 0x43505646u   /* "FVPC" */
#define FOVPT_PACKET_RAW     0u
#define FOVPT_PACKET_BC1     1u
#define FOVPT_PACKET_BY_FILL 0xffffffffu       /* in a config only: BC1 where the pass's fill > 1 */
typedef struct fovpt_packet_config {    /* 16 bytes */
    uint32_t codec[3];                  /* per launch pass (P, M, F; FOV_OFF: one) */
    uint32_t _reserved;                 /* 0 */
} fovpt_packet_config;
void fovpt_packet_defaults(fovpt_packet_config* cfg);
int fovpt_packet_describe_coded(fovpt_ctx* ctx, const fovpt_launch_params* lp, const fovpt_packet_config* cfg, uint32_t sequence,
                                fovpt_packet_header* out);
int fovpt_packet_encode_coded(fovpt_ctx* ctx, const fovpt_launch_params* lp, const fovpt_packet_config* cfg, const uint32_t* in_rgba,
                              uint32_t sequence, void* out_packet);
int fovpt_packet_submit_coded(fovpt_ctx* ctx, const fovpt_launch_params* lp, const fovpt_packet_config* cfg, const uint32_t* in_rgba,
                              uint32_t sequence, int* slot);

/* ---- depth packets and late reprojection on the client ---------------------------------------------------------------------------
 * New with this library (the definitions: tests/packet_depth_ref.py, tests/warp_depth_ref.py).  A colour
 * packet shows the frame at the pose it was rendered for.  A depth packet ("FVPD") carries the frame's depth the way the colour
 * travels -- one value per launch index -- together with the rendered camera, so that a client which holds no scene decodes both
 * and re-aims the image itself: fovpt_packet_decode (colour), fovpt_packet_decode_depth, fovpt_warp_depth, fovpt_lens.
 *   layout    fovpt_packet_depth_header (192 bytes: a fovpt_packet_header with magic "FVPD", version 1 and the pass records of
 *             the colour packet of the same frame, their eighth word 0; then eye, U, V, W of the rendered camera, `near`, three
 *             zero words), then per pass gw * gh uint16 codes, row-major ly * gw + lx, and 0 or 2 zero bytes so that the next
 *             array starts at a multiple of 4; the arrays lie back to back from byte 192.  Little endian.  `bytes` is the whole
 *             packet, padding included.
 *   code      of a pixel, from the G-buffer's prim and position.xyz, every *, +, - and / one unfused binary32 operation, M the
 *             rows of inverse([U V W]) of the rendered camera as fovpt_warp computes them for `to` (binary64, rounded to fp32):
 *               prim == 0xffffffff: 1 (sky, at infinity).  Else v = X - eye, z = (M_2.x v.x + M_2.y v.y) + M_2.z v.z -- the point
 *               is eye + z * pixel_ray(x, y): no square root --; !(z > 0) or z not finite: 1; else q = near / z,
 *               c = floorf(q * 65534.0f + 0.5f) clamped in float to [1, 65534], code = (uint32)c + 1: hits are 2 .. 65535.
 *             of a texel: 0 where the launch index owns no pixel (ownership: fovpt_packet_encode's), else the LARGEST code of the
 *             pixels it owns -- the nearest surface, which a disocclusion must not lose; sky only where every owned pixel is sky.
 *   decode    one mode: a pixel takes the last texel with code != 0 whose block reaches it (the colour decoders' search with
 *             "code != 0" for "alpha != 0"); out_depth = +inf for code 1, else (near * 65534.0f) / (float)(code - 1); a pixel
 *             no texel reaches keeps what the output held.
 *   fovpt_packet_depth_defaults   near 0.1f (a convention, not a measurement): depths below it saturate at code 65535.
 *   fovpt_packet_describe_depth / _encode_depth / _submit_depth   ordering, validation and error codes of fovpt_packet_encode /
 *             _submit (a frame rendered whole at lp's size, world == 1, a 4-byte-aligned buffer, written whole and nothing else),
 *             the same four slots and copy stream (colour, coded and depth submits may alternate; fovpt_packet_wait serves all).
 *             gbuffer as fovpt_warp takes it: NULL traces into fovpt_gbuffer's buffers and needs the scene (FOVPT_E_NO_SCENE),
 *             non-NULL is used as given -- only prim and position are read, the size must be the frame's.  Additionally
 *             FOVPT_E_INVALID for a null cfg, a non-zero reserved word, a `near` that is not finite and above 0, a singular or
 *             non-finite rendered camera.  k_packet_depth_encode: one thread per texel, a 2-byte store each, no atomics, no LDS.
 *   fovpt_packet_check_depth / _decode_depth_host   no context, both libraries.  FOVPT_E_INVALID for everything fovpt_packet_check
 *             rejects with 192 in the place of 128 and an array's end offset + 2 gw gh rounded up to 4 (in 64 bits) above `bytes`;
 *             a non-zero eighth pass word; a non-finite camera entry; a [U V W] whose determinant is 0 or not finite; `near` not
 *             finite or not above 0; non-zero words 45 .. 47; an output of another size; null pointers.  fovpt_packet_check,
 *             fovpt_packet_decode and fovpt_packet_decode_host refuse the magic "FVPD".
 *   fovpt_packet_decode_depth     device decoder (k_packet_depth_decode, one thread per pixel) on fovpt_stream(): header on the
 *             host, packet (4-byte aligned) and out_depth (header's width x height floats) on the device.  Needs no rendered frame
 *             and no scene: a context fresh from fovpt_create does.  The reach limit of fovpt_packet_decode.
 *   fovpt_warp_depth              fovpt_warp, operation for operation -- the key, the landing test, the depth word, the resolve,
 *             the classes, the map, the counts, images and fill_radius --, with the source point rebuilt from a depth image and
 *             the camera `from` it was rendered with; needs no rendered frame and no scene.  Per source pixel s = y * w + x,
 *             z = depth[s]:  z == +inf: a miss, v = pixel_ray(from; x, y) = (dx U + dy V) + W, dx = 2 ((x + 0.5) / w) - 1, depth
 *             word 0x7fffffff;  z finite and above 0: r = pixel_ray(from; x, y), X_k = eye_from_k + z * r_k, v = X - eye_to, then
 *             fovpt_warp's a_k, px, py, fx, fy and key;  anything else (NaN, <= 0, -inf): the pixel scatters nothing.  With
 *             to == from every pixel with a finite positive or infinite depth lands on itself (tests/test_warp_depth_cpu.py).
 *             The keys are the context's own for this call (width x height, grown on demand; not fovpt_warp's);
 *             fovpt_warp_counts reports the last warp of any of the three kinds.  The outputs of enabled images are the caller's.
 *             FOVPT_E_INVALID: null ctx / from / to / wc / depth; width or height below 1 or width * height >= 2^30; fovpt_warp's
 *             checks on images, fill_radius and reserved fields, and on `to`, applied to `from` as well; an enabled image with a
 *             null input or output; any output equal to any input, to depth or to another output.
 * Out of scope.  Smoothing or predicting depth (a texel is one surface's); a codec for the depth plane; moving meshes
 * (fovpt_warp_motion needs the server's hit records).
 * A 1920 x 1080 frame at radii 148 / 482 has 452 660 launch indices: 905 512 bytes of depth beside the colour packet's 1 810 768.
 * The times of these calls have not been measured on an MI355X yet; tools/packet_perf.py --depth measures them (DESIGN.md,
 * section 39).                                                                                                                      */
#define FOVPT_PACKET_MAGIC_DEPTH 0x44505646u   /* "FVPD" */
#define FOVPT_PACKET_DEPTH_HEADER_BYTES 192
typedef struct fovpt_packet_depth_config {  /* 16 bytes */
    float near;                         /* finite, above 0; default 0.1f: depths below it saturate (a convention, not a measurement) */
    uint32_t _reserved[3];              /* 0 */
} fovpt_packet_depth_config;
typedef struct fovpt_packet_depth_header {  /* 192 bytes */
    fovpt_packet_header base;           /* magic "FVPD"; texels: byte offset of a pass's code array, >= 192 */
    fovpt_warp_camera camera;           /* the camera the frame was rendered with */
    float near;
    uint32_t _reserved[3];              /* 0 */
} fovpt_packet_depth_header;
void fovpt_packet_depth_defaults(fovpt_packet_depth_config* cfg);
int fovpt_packet_describe_depth(fovpt_ctx* ctx, const fovpt_launch_params* lp, const fovpt_packet_depth_config* cfg, uint32_t sequence,
                                fovpt_packet_depth_header* out);
int fovpt_packet_encode_depth(fovpt_ctx* ctx, const fovpt_launch_params* lp, const fovpt_packet_depth_config* cfg,
                              const fovpt_gbuffer_ptrs* gbuffer /* NULL: traced by the call */, uint32_t sequence, void* out_packet);
int fovpt_packet_submit_depth(fovpt_ctx* ctx, const fovpt_launch_params* lp, const fovpt_packet_depth_config* cfg,
                              const fovpt_gbuffer_ptrs* gbuffer /* NULL: traced by the call */, uint32_t sequence, int* slot);
int fovpt_packet_check_depth(const void* packet, size_t bytes);
int fovpt_packet_decode_depth_host(const void* packet, size_t bytes, float* out_depth, int width, int height);
int fovpt_packet_decode_depth(fovpt_ctx* ctx, const fovpt_packet_depth_header* header /* host */, const void* packet /* device */,
                              float* out_depth /* device, header's width x height */);
int fovpt_warp_depth(fovpt_ctx* ctx, int width, int height, const fovpt_warp_camera* from, const fovpt_warp_camera* to,
                     const fovpt_warp_config* wc, const float* depth, const fovpt_float4* in_color, const uint32_t* in_rgba,
                     fovpt_float4* out_color, uint32_t* out_rgba, uint32_t* out_map /* may be NULL */);

/* ---- multi-GPU: packed gather of the final framebuffer ----------------------------------
 * New with this library: the reference is single-GPU (SimplePathtracer.cpp:331-340).  With
 * fovpt_config.rank/world every handle renders the launch-index tiles it owns -- interleaved
 * 8 x 4 tiles dealt round-robin, the scheme of the SDK's unused sutil/WorkDistribution.h:47-84
 * -- so the pixels of a frame partition by the owner of their last writer.
 *   fovpt_gather_plan    builds (or reuses) the partition for the frame fovpt_render would
 *                        draw with the current config and lp (frame size, gaze): per rank the
 *                        ascending list of pixel indices it owns; counts_out[r] = their number.
 *                        Every rank computes the same plan.  Synchronises when it rebuilds.
 *   fovpt_gather_pack    copies THIS rank's owned rgba8 words of `frame` into `packed`
 *                        (counts[rank] words), in plan order; asynchronous on fovpt_stream().
 *   fovpt_gather_unpack  scatters `world` packed buffers (rank r's at gathered + r * stride)
 *                        into `frame`; pixels nobody owns are left untouched; asynchronous.
 * Between pack and unpack the caller moves the buffers with RCCL (gather to the root over xGMI:
 * 1/world of the frame per rank instead of a full-frame reduce).  All pointers are device
 * pointers.                                                                                */
int fovpt_gather_plan(fovpt_ctx* ctx, const fovpt_launch_params* lp, uint32_t* counts_out, int counts_len);
int fovpt_gather_pack(fovpt_ctx* ctx, const uint32_t* frame, uint32_t* packed);
int fovpt_gather_unpack(fovpt_ctx* ctx, const uint32_t* gathered, uint32_t stride, uint32_t* frame);

/* ---- multi-GPU: the RCCL transport of that gather, for C / C++ hosts ----------------------
 * One fovpt_ctx per GPU (one process or thread each), fovpt_config.rank / world set on each.
 *   fovpt_comm_get_unique_id  ncclGetUniqueId: one rank creates the 128-byte id and hands it to the others out of band
 *                             (MPI_Bcast, a file, a socket: the host application's business)
 *   fovpt_comm_init           ncclCommInitRank on the context's device; collective over all ranks
 *   fovpt_gather_frame        plan (cached) -> pack -> ncclGroupStart / ncclSend to `root` / on the root ncclRecv from every
 *                             rank / ncclGroupEnd -> on the root unpack into full_frame.  Everything is enqueued on
 *                             fovpt_stream(): asynchronous, ordered behind the frame just rendered, and running beside the
 *                             next frame's rendering.  `frame` is this rank's rgba8 frame (what fovpt_render wrote);
 *                             full_frame (root only; may be `frame` itself) receives the whole image.
 *   fovpt_comm_destroy        ncclCommDestroy (also done by fovpt_destroy)
 * librccl is loaded at run time (dlopen: $FOVPT_RCCL_LIB, librccl.so.1, librccl.so); without it these return
 * FOVPT_E_DEVICE and everything else in this header works.  Replaces nothing in the reference (single-GPU,
 * SimplePathtracer.cpp:331-340); the partition is the scheme of sutil/WorkDistribution.h:47-84.                        */
#define FOVPT_COMM_ID_BYTES 128
int fovpt_comm_get_unique_id(void* id);
int fovpt_comm_init(fovpt_ctx* ctx, const void* id, int rank, int world);
int fovpt_comm_destroy(fovpt_ctx* ctx);
int fovpt_gather_frame(fovpt_ctx* ctx, const fovpt_launch_params* lp, int root, const uint32_t* frame, uint32_t* full_frame);

/* CUDA_SYNC_CHECK() (SimplePathtracer.cpp:212). */
int fovpt_synchronize(fovpt_ctx* ctx);

/* CUDABuffer::download (CUDABuffer.h:82-88): device -> host copy of n_bytes.      */
int fovpt_download(fovpt_ctx* ctx, const void* device_src, void* host_dst, size_t n_bytes);

int fovpt_get_stats(fovpt_ctx* ctx, fovpt_stats* out);   /* synchronises first */
int fovpt_reset_stats(fovpt_ctx* ctx);
/* hipStream_t; SampleRenderer::stream.  Frames complete on it in submission order: work
 * queued on it after fovpt_render / fovpt_launch sees the finished frame and is ordered
 * before the next frame's writes to the render target.                              */
void* fovpt_stream(fovpt_ctx* ctx);

/* ---- host-side helpers that the reference runs on the CPU too ---------------- */
/* ProbeData::BuildCDF (Probe.h:29-77): sequential fp32 accumulation, order preserved. */
int fovpt_probe_build_cdf(int width, int height, const fovpt_float4* data,
                          float* pdfValuesX, float* cdfValuesX,
                          float* pdfValuesY, float* cdfValuesY);
/* sutil::Camera::UVWFrame (sutil/Camera.cpp:32-44). */
int fovpt_camera_uvw(const fovpt_float3* eye, const fovpt_float3* lookat, const fovpt_float3* up,
                     float fovY_degrees, float aspect,
                     fovpt_float3* U, fovpt_float3* V, fovpt_float3* W);

/* ---- Scene ingestion on the host: what loadOBJ returns, PT_sv5_/Model.cpp:138-217 --------------------
 * (with addVertex :49-82 and loadTexture :84-136, i.e. the vendored tinyobjloader with triangulate = true and
 * stbi_load(..., STBI_rgb_alpha) mirrored along y).  Plain host code, no GPU needed.  One mesh per (shape, material id);
 * PNG, JPEG, Truevision TGA and binary PPM textures are decoded, any other format counts as "could not load"
 * (texture id -1, as :129-131).
 * The arrays stay owned by the model; include/Model.h wraps this as `Model* loadOBJ(const std::string&)`.
 * Errors: FOVPT_E_INVALID, text from fovpt_last_error(NULL) ("Could not read OBJ model from ...", :160-162).          */
typedef struct fovpt_model fovpt_model;
typedef struct fovpt_model_mesh {
    const fovpt_float3* vertex;      /* TriangleMesh::vertex                                   */
    const fovpt_float3* normal;      /* TriangleMesh::normal, NULL when the mesh has none      */
    const float* texcoord;           /* TriangleMesh::texcoord as (u, v) pairs, NULL when none */
    const fovpt_uint3* index;        /* TriangleMesh::index                                    */
    uint32_t num_vertices, num_normals, num_texcoords, num_triangles;
    fovpt_material material;         /* reference defaults + Kd -> color, Ke -> emission (:190-191) */
    int32_t diffuse_texture_id;      /* index into the model's textures, or -1                 */
} fovpt_model_mesh;
int fovpt_model_load_obj(const char* obj_file, fovpt_model** out);
/* glTF 2.0 (.gltf with external or data-URI buffers, or a .glb container) -> the same model structure, one mesh per triangle
 * primitive in WORLD space, with the node rules of sutil::Scene (sutil/Scene.cpp:109-442: roots = nodes without a parent,
 * parent * matrix * T * R * S in binary32, nothing below a mesh or camera node, base colour / roughness / metallic factors,
 * emissiveFactor -> emission, base colour texture from a PNG / TGA / PPM file).  Replaces tinygltf + sutil::loadScene for C++
 * callers; include/Model.h wraps it as `Model* loadGLTF(const std::string&)`.                                            */
int fovpt_model_load_gltf(const char* gltf_file, fovpt_model** out);
void fovpt_model_destroy(fovpt_model* model);
int fovpt_model_counts(const fovpt_model* model, int* num_meshes, int* num_textures);
int fovpt_model_get_mesh(const fovpt_model* model, int i, fovpt_model_mesh* out);
int fovpt_model_get_texture(const fovpt_model* model, int i, const uint32_t** pixels, int* width, int* height);

/* The float4 texels loadProbe hands to ProbeData::BuildCDF (PT_sv5_/main.cpp:160-171): what
 * stbi_loadf(file, &w, &h, &n, 4) returns -- Radiance .hdr as it is (RLE and flat scanlines, alpha 1), 8-bit PNG / TGA /
 * PPM through stb's gamma-2.2 conversion.  *texels is malloc'ed, width * height entries, row 0 first; release it with
 * fovpt_image_free.  Errors: FOVPT_E_INVALID with fovpt_last_error(NULL) (the reference does not check stbi_loadf's
 * result and would build the CDF over a null pointer).                                                               */
int fovpt_image_load_float4(const char* file, int* width, int* height, fovpt_float4** texels);
/* stbi_load(file, &w, &h, &n, STBI_rgb_alpha) as loadTexture calls it (PT_sv5_/Model.cpp:106-107) for the formats this library
 * reads -- PNG, JPEG (baseline, extended, progressive; gray, YCbCr, RGB, CMYK, YCCK), Truevision TGA, binary PPM: rgba8, row 0
 * first, bit for bit what the reference's vendored stb_image returns.  *pixels is malloc'ed: fovpt_image_free_rgba8.           */
int fovpt_image_load_rgba8(const char* file, int* width, int* height, uint32_t** pixels);
void fovpt_image_free_rgba8(uint32_t* pixels);
void fovpt_image_free(fovpt_float4* texels);

/* ---- device self-test hook (tests only): evaluates one scalar function on the GPU
 * for n inputs; op codes FOVPT_OP_*.  a,b host arrays (b may be NULL), out host.
 * The functions of fovpt_detmath.h keep their domains here (nothing is checked): SIN / COS |a| <= 2^20; ACOS a in [-1, 1];
 * ATAN2 (y = a, x = b) finite operands; LOG every binary32; POW (x = a, y = b) a >= 0 finite or NaN, any b, a = +inf
 * excluded.  Outside them the result is undefined and need not equal the host's.  SQRT and DIV are the hardware's IEEE
 * operations on every binary32.                                                     */
#define FOVPT_OP_SIN    1
#define FOVPT_OP_COS    2
#define FOVPT_OP_ACOS   3
#define FOVPT_OP_ATAN2  4
#define FOVPT_OP_LOG    5
#define FOVPT_OP_POW    6
#define FOVPT_OP_SQRT   7
#define FOVPT_OP_DIV    8
#define FOVPT_OP_RSQRTD 9   /* (float)(1.0 / (double)sqrtf(a)), maths.h:98 */
#define FOVPT_OP_UNORM8 10  /* texel channel (uint8)a / 255.0f as the shading kernel computes it */
#define FOVPT_OP_HALFPLUS 11 /* (float)(0.5 + (double)a), Disney.cuh Fd90 */
int fovpt_debug_math(fovpt_ctx* ctx, int op, const float* a, const float* b, float* out, size_t n);
/* tests only: the production traversal kernel on a batch of n rays (host arrays, 3 floats per origin / direction): closest
 * hit -> global primitive id (0xffffffff = miss) and (t, u, v); occlusion ray (deviceProgram.cu:224-248) -> 0 / 1.
 * Any output may be NULL.  Synchronises.                                                                              */
int fovpt_debug_trace(fovpt_ctx* ctx, int n, const float* origins3, const float* dirs3, uint32_t* prim_out, float* tuv_out3, uint8_t* occluded_out);
/* tests only: the production traversal launches -- closest hit, then occlusion, each as a job launches it -- on a queue state the
 * caller lays out, and everything they left, so that the kernel's QUEUE side (which shards a launch reads, the map from a queue
 * index to its place, where a hit record and a shadow result go, which counter words are read) can be held against the oracle
 * ray by ray.  fovpt_debug_trace is this call with every ray in shard 0, slot = index, cell 0 and the production grids.
 *
 * In (host arrays): n rays (origins3, dirs3); per ray its sample slot (slot: a permutation of 0 .. n-1), the target of its shadow
 * record (target: a radiance cell 0 .. max_depth-1, or FOVPT_DEBUG_TRACE_ALPHA: the slot's alpha) and the two records of the
 * shadow queue (vis4, occ4: four floats each; the launch stores .xyz of one of them and +0).  Every ray is in BOTH queues, at the
 * same index: q_count[s] / sq_count[s] = how many of the rays, taken in order, lie in shard s of the radiance / the shadow queue.
 * sel = 0 (all eight shards) or 1 / 2 (the first / second four: a chain of a job); with sel != 0 the other four shards may hold
 * the other chain's live rays, other_* (n_other of them, slots a permutation of n .. n+n_other-1), whose counts stand in the same
 * counter words; both != 0 runs the other chain's two launches behind this one's, on the same stream and the same state.
 * it_closest / it_shadow = the iterations whose counter words hold the counts (0 .. FOVPT_DEBUG_TRACE_ITERS-1); decoy[s] is
 * written into every other word of shard s that a neighbouring iteration would use -- radiance it_closest +- 1 and it_shadow,
 * shadow it_shadow +- 1 and it_closest.  grid_closest / grid_shadow = the launcher's grid argument (units of 256 threads), 0 =
 * what a job of this sel uses.  slots sizes the queues as a job of that many sample slots would (0 = 8 * max(n, 1)): cap = the
 * capacity of a shard.
 * Before the launch the hit buffer (8 * cap entries) and the cells and alpha of n + n_other + 1 sample slots hold the byte
 * FOVPT_DEBUG_SHADE_FILL, and every queue entry no ray occupies holds one fixed ray (from the middle of the scene along +y) whose
 * shadow record names cell 0 of the last slot, n + n_other: the trap slot no ray owns.
 * Out (host arrays of the caller's): the hit-buffer entries that differ from the fill, wherever they lie -- hit_found of them,
 * the first n + n_other in ascending physical order as (shard, position) in hit_place2, the record in hit4 and its global
 * primitive id (0xffffffff = miss) in hit_prim; cells4 = max_depth float4 per slot and alpha4 = one, of all n + n_other + 1
 * slots; the rise of the three ray statistics; counters_changed = queue counter words that are not what was written;
 * queues_unchanged = 1 when all six queue arrays are byte for byte what was uploaded; cap.
 * Errors: FOVPT_E_NO_SCENE, FOVPT_E_INVALID (counts that do not sum to n or n_other, exceed cap or lie outside their selection;
 * slots that are no permutation; a target, an iteration, a grid or sel out of range), FOVPT_E_DEVICE (a hit record that names
 * no triangle).  Synchronises.                                                                                             */
#define FOVPT_DEBUG_TRACE_ALPHA 0xffffffffu
#define FOVPT_DEBUG_TRACE_ITERS 63
typedef struct fovpt_debug_trace_launch {
    const float *origins3, *dirs3;
    const uint32_t *slot, *target;
    const float *vis4, *occ4;
    const float *other_origins3, *other_dirs3;
    const uint32_t *other_slot, *other_target;
    const float *other_vis4, *other_occ4;
    int32_t n, n_other;
    uint32_t sel, both;
    int32_t it_closest, it_shadow, grid_closest, grid_shadow;
    uint32_t slots;
    uint32_t q_count[8], sq_count[8], other_q_count[8], other_sq_count[8], decoy[8];
} fovpt_debug_trace_launch;
typedef struct fovpt_debug_trace_result {
    uint32_t *hit_place2;
    float *hit4;
    uint32_t *hit_prim;
    float *cells4, *alpha4;
    uint64_t stat_radiance, stat_shadow, stat_paths;
    uint32_t hit_found, counters_changed, queues_unchanged, cap;
} fovpt_debug_trace_result;
int fovpt_debug_trace_queued(fovpt_ctx* ctx, const fovpt_debug_trace_launch* launch, fovpt_debug_trace_result* out);
/* tests only: the device functions of a shaded hit on n inputs the caller chose (host arrays), so that the probe lookup, the
 * Disney BSDF and the texture fetch can be compared with the oracle input by input.  All synchronise; any output may be NULL.
 *
 * fovpt_debug_probe_sample: ProbeSample (Probe.cuh:138-169) with its two random numbers given, r12 = n pairs in Randf's range
 *   [0, 0.999999] -> the row and column the two searches found (rowcol_out2) and direction.xyz, colour.xyz, pdf (out7).
 *   As for a launch, the last entry of cdfValuesY and of every row of cdfValuesX must be at least 0.999999 (BuildCDF ends
 *   them at 1): a search for a number above a row's last entry returns the row's length, and the lookup reads past the row.
 * fovpt_debug_probe_eval: ProbeDirToUV + ProbeEval, the backplate of the raygen program -> u, v, texel.xyzw (out6).
 *   `probe` is what a launch takes (device pointers).  The arrays are searched and read the way a launch of this context
 *   would: *path_out tells how (FOVPT_PROBE_PATH_* bits; 0 = the reference's plain binary search over all rows).
 *   flags = FOVPT_DEBUG_PROBE_PLAIN forces that plain path on the same arrays.
 * fovpt_debug_bsdf: per row BasisFromVector(N), then with Random(seed) BSDFSample and -- if its pdf is above 0 -- BSDFEval and
 *   BSDFPdf at the sampled direction, then BSDFPdf and BSDFEval at L_given (the next-event branch: a direction from the
 *   probe, which may lie below the surface) -> out14 = light.xyz, pdf, eval.xyz, pdf_again, the generator's two state words
 *   afterwards (as bits), eval_given.xyz, pdf_given.
 * fovpt_debug_tex2d: the bilinear wrap-addressed fetch of texture `texture` of the current scene at n (u, v) -> rgba.       */
#define FOVPT_DEBUG_PROBE_PLAIN   1
#define FOVPT_PROBE_PATH_GUIDED   1   /* both searches go through the guide tables                                  */
#define FOVPT_PROBE_PATH_RECORDS  2   /* column search, pdf and colour from the packed 32-byte records               */
#define FOVPT_PROBE_PATH_ONE_ROW  4   /* all rows alike: served from row 0 (row_mul = 0)                             */
int fovpt_debug_probe_sample(fovpt_ctx* ctx, const fovpt_probe* probe, int flags, int n, const float* r12, int32_t* rowcol_out2, float* out7, int* path_out);
int fovpt_debug_probe_eval(fovpt_ctx* ctx, const fovpt_probe* probe, int flags, int n, const float* dirs3, float* out6, int* path_out);
int fovpt_debug_bsdf(fovpt_ctx* ctx, const fovpt_material* material, int n, const float* N3, const float* view3, const float* albedo3, const float* etaI,
                     const float* etaO, const int32_t* seeds, const float* L_given3, float* out14);
int fovpt_debug_tex2d(fovpt_ctx* ctx, int texture, int n, const float* uv2, float* rgba_out4);
/* tests only: the production shading kernel on n hits the caller made (host arrays), launched once as a job launches it -- with
 * the configured max_depth, options (which pick the kernel's build) and write_guides --, and what it left.
 *
 * Per hit i (= sample slot i): origin3, dir4 = ray direction and, in .w, the pdf of the sample that sent the ray; prim = global
 * primitive id or 0xffffffff for a miss, with tuv3 = (t, u, v); rng3 = the slot's generator words s1, s2 and flags | depth << 8;
 * thr4 = pathThroughput.xyz and rayEta.  `probe` is what a launch takes (device pointers) and is searched as a launch would.
 * The launch: depth_iter = the iteration whose queue the hits are (they are appended to the queues of depth_iter + 1 and of
 * depth_iter's shadow rays), sel = 0 (all eight queue shards) or 1 / 2 (the first / second four), grid = blocks,
 * partition = the direction classes of foveated frames, shard_count[s] = how many of the hits, taken in order, lie in input
 * shard s.  The state is sized so that any one shard can hold all n entries: cap = the capacity of a shard.
 * Out, per slot: rng4, thr4, rad4 (max_depth cells), alpha4, guide_n4 / guide_a4 (under write_guides).  The counters of the next
 * queue and of the shadow queue per shard; *_found = the entries of those queues that differ from the fill pattern (every byte
 * FOVPT_DEBUG_SHADE_FILL), wherever they lie; the first n of them in ascending physical order with (shard, position) in
 * *_place2.  counters_changed = other counter words that changed.  Every out array has room for n entries.
 * Errors: FOVPT_E_NO_SCENE, FOVPT_E_NO_PROBE, FOVPT_E_INVALID.                                                              */
#define FOVPT_DEBUG_SHADE_FILL 0xcd
typedef struct fovpt_debug_shade_launch {
    int32_t n, depth_iter, grid, partition;
    uint32_t sel;
    uint32_t shard_count[8];
} fovpt_debug_shade_launch;
typedef struct fovpt_debug_shade_result {
    uint32_t *rng4;
    float *thr4, *rad4, *alpha4, *guide_n4, *guide_a4;
    uint32_t *next_place2;
    float *next_o4, *next_d4;
    uint32_t *shadow_place2;
    float *shadow_o4, *shadow_d4, *shadow_vis4, *shadow_occ4;
    uint32_t next_count[8], shadow_count[8];
    uint32_t next_found, shadow_found, counters_changed, cap;
} fovpt_debug_shade_result;
int fovpt_debug_shade(fovpt_ctx* ctx, const fovpt_probe* probe, const fovpt_debug_shade_launch* launch, const float* origin3, const float* dir4,
                      const uint32_t* prim, const float* tuv3, const uint32_t* rng3, const float* thr4, fovpt_debug_shade_result* out);
/* tests only: the production resolve kernel on a path state the caller made, so that the last-writer search, the ordered sums,
 * the alpha flags, the backplate mix, accumulate mode, the tone map and the tile ownership of a sharded frame can be compared
 * with a restatement pixel by pixel and case by case, not only through rendered frames.
 *
 * The frame is the one fovpt_launch(lp, width, height) (render = 0) or fovpt_render(lp) (render = 1; width and height unused)
 * would resolve under the current configuration; lp is not changed.  passes_out (room for 3) / npass_out: the passes in launch
 * order with their places in the arrays -- sample slot of (pass, launch index li = ly * gw + lx, sample s) =
 * slot_base + li * spp + s, launch record = launch_base + li.  With state = NULL the call returns after filling them.
 * Otherwise, host arrays in slot order: state = flags | depth << 8 (DONE 1, SECONDARY 2, ALPHA_ONE 4, ALPHA_SET 8), cells4 =
 * max_depth float4 radiance cells per slot, alpha4 = float4 per slot, guide_n4 / guide_a4 = float4 per slot (read under
 * write_guides only, may be NULL otherwise), backplate4 = float4 per launch record.  The call uploads them, runs the kernel
 * and synchronises; the caller reads its own frame buffers.  *counters_left_out: how many words of the state set's queue
 * counters -- filled with a pattern before the launch -- the kernel left non-zero (a resolve zeroes them for the next job).
 * Errors: FOVPT_E_NO_FRAME, FOVPT_E_INVALID (also: a frame that would run as several jobs).                              */
typedef struct fovpt_debug_pass { uint32_t gw, rows, spp, slot_base, launch_base; } fovpt_debug_pass;
int fovpt_debug_resolve(fovpt_ctx* ctx, const fovpt_launch_params* lp, int render, uint32_t width, uint32_t height, fovpt_debug_pass* passes_out,
                        int* npass_out, const uint32_t* state, const float* cells4, const float* alpha4, const float* guide_n4, const float* guide_a4,
                        const float* backplate4, uint32_t* counters_left_out);
/* tests only: the production generate launch -- k_generate, or k_generate_owned for a rank of a tile-sharded frame, whichever the
 * library's launcher picks -- so that seeding, jitter, camera rays, backplates, the slot-to-launch decode, the ring test, tile
 * ownership and the sharded queue can be compared with the oracle and a restatement slot by slot, not only through frames.
 *
 * The frame is the one fovpt_launch(lp, width, height) (render = 0) or fovpt_render(lp) (render = 1; width, height, row0, row1
 * unused and 0) would run under the current configuration (world, rank, tile_w, tile_h, write_guides, uniform, max_depth); lp is
 * not changed.  With render = 0 and row1 > 0 the job is the chunk of launch rows [row0, row1) of that launch, as an oversized
 * launch is cut: sample slots and launch records are then relative to the chunk.  passes_out (room for 3) / npass_out are
 * fovpt_debug_resolve's; with out = NULL the call returns after filling them.
 * The launch: sel = 0 (all eight queue shards) or 1 / 2 (the first / second four: one of the two chains of a job), the sample
 * slots [slot_begin, slot_end) -- 0 / 0: all of them for sel = 0, the half that a job's chain of that sel takes otherwise --
 * and grid = blocks, a positive multiple of 8 (of 4 with sel != 0), or 0: what a job uses.  What ran is reported in out.
 * The state is sized as a job sizes it (cap = the capacity of a queue shard), except that queue 0 is a scratch queue of
 * 8 * cap + slots + 256 entries: a shard that overflows shows in the result and nothing else is overwritten.  The generator
 * words, the backplates, the guides and the scratch queue are filled with the byte FOVPT_DEBUG_SHADE_FILL before the launch and
 * the queue counters are zero, as a job finds them.
 * Out, host arrays of the caller's: rng4 per sample slot, backplate4 per launch record, guide_n4 / guide_a4 per slot (under
 * write_guides only: guides = 1; otherwise they are not touched and may be NULL), count[s] = the counter of queue 0 in shard
 * s, counters_changed = other counter words that are not zero, found = the entries of the scratch queue that differ from the
 * fill pattern, wherever they lie; the first `slots` of them in ascending physical order with (shard, position) in place2 (an
 * entry behind the eighth shard reports a shard of 8 or more), origin and slot in o4, direction in d4 (room for `slots` entries
 * each).  kernel = 0: k_generate ran, 1: k_generate_owned.
 * Errors: FOVPT_E_NO_FRAME, FOVPT_E_NO_PROBE, FOVPT_E_INVALID (also: a frame that would run as several jobs).             */
typedef struct fovpt_debug_generate_launch {
    int32_t render;
    uint32_t width, height, row0, row1;
    uint32_t sel, slot_begin, slot_end;
    int32_t grid;
} fovpt_debug_generate_launch;
typedef struct fovpt_debug_generate_result {
    uint32_t *rng4;
    float *backplate4, *guide_n4, *guide_a4;
    uint32_t *place2;
    float *o4, *d4;
    uint32_t count[8];
    uint32_t found, counters_changed, cap, kernel, guides, slot_begin, slot_end, grid;
} fovpt_debug_generate_result;
int fovpt_debug_generate(fovpt_ctx* ctx, const fovpt_launch_params* lp, const fovpt_debug_generate_launch* launch, fovpt_debug_pass* passes_out,
                         int* npass_out, fovpt_debug_generate_result* out);
/* tests only: the production hierarchy build (the function fovpt_set_scene and every rebuild call) over n triangles the caller
 * supplies (host array, 9 floats each; mesh_of_prim: a mesh id per triangle, NULL = all 0), under explicit switches -- nothing is
 * read from the environment --, and what every stage of it left, so that splits, boxes, Morton keys, the sort, the binary tree,
 * reinsertion, the collapse's dynamic programme, the emitted wide tree and the child order can each be held against a
 * restatement, not only the rays a finished tree answers.  Needs no scene and leaves the context as it was.  Synchronises.
 *
 * Switches: use_ploc (0: the plain Karras tree), split_budget in [0, 2] (0: no spatial splits), reinsert_rounds >= 0 (PLOC only),
 * order_children (0: keep the collapse's child order).
 * The trace, arrays of the caller's (any may be NULL = not asked for).  R = num_refs, the build primitives: the triangles, or
 * their references under splits; cap_refs (in) = the room of every per-reference array, R <= n * (1 + split_budget); when
 * cap_refs < R the call sets num_refs, writes no array and returns FOVPT_E_INVALID.  I = R - 1 internal nodes of the binary
 * tree, whose children are coded >= 0: internal node, < 0: ~(sorted position of a leaf).
 *   split_count, split_first (n; written when split_budget > 0 and n > 4: have_count = 1), ref_prim (R; have_splits = 1 only),
 *   boxes (R x 6: lo.xyz, hi.xyz), cbounds (the centroid bounds min.xyz, max.xyz), vals_s (R), leaf_pos (R), nodes_pre = the
 *   wide nodes before the child order (num_nodes x 32 words), nodes and tris = the result (num_nodes x 32, R x 12 words),
 *   level_first (num_levels + 1) -- always;
 *   keys_s (R), left0 / right0 (I), ibox0 (I x 6), root, round_end (num_rounds <= cap_rounds (in) entries; PLOC only) = the
 *   tree as PLOC or Karras left it, left1 / right1 / ibox1, size_int, node_first (I) = the tree the collapse saw, dp (I x 4
 *   words: c1, c2, c3 as float bits, dec) -- unless tiny = 1 (R <= 4: one root with one leaf, no keys, no binary tree).       */
typedef struct fovpt_debug_build_switches {
    int32_t use_ploc;
    float split_budget;
    int32_t reinsert_rounds, order_children;
} fovpt_debug_build_switches;
typedef struct fovpt_debug_build_trace {
    uint32_t *split_count, *split_first, *ref_prim;
    float *boxes;
    uint64_t *keys_s;
    uint32_t *vals_s;
    int32_t *left0, *right0;
    float *ibox0;
    uint32_t *round_end;
    int32_t *left1, *right1;
    float *ibox1;
    uint32_t *size_int, *node_first, *leaf_pos, *dp, *nodes_pre, *nodes, *tris;
    uint32_t cap_refs, cap_rounds;
    uint32_t num_refs, tiny, have_count, have_splits, root, num_rounds, num_nodes, max_depth, reinserted, num_levels;
    float s_cut;
    float cbounds[6];
    uint32_t level_first[65];
} fovpt_debug_build_trace;
int fovpt_debug_build(fovpt_ctx* ctx, uint32_t n, const float* tris9, const uint32_t* mesh_of_prim, const fovpt_debug_build_switches* switches,
                      fovpt_debug_build_trace* trace);
/* tests/diagnostics only: device address and size of an internal buffer ("sq_occ", "counters", "hit", "bvh_nodes", "bvh_tris"
 * -- the 48-byte triangle records of the hierarchy, stats.tri_bytes --, "scene_vertices" -- fovpt_update_vertices' vertex
 * array, once made --, "scene_vertices_prev" -- fovpt_temporal_motion's previous positions, once made --, "gbuffer_hit" -- the
 * hit records of the last G-buffer trace (fovpt_gbuffer, fovpt_reconstruct, a temporal step): float4 (t, u, v, record offset
 * as bits, 0xffffffff on a miss) per pixel --, "expose_histogram" -- fovpt_expose's last metered histogram, FOVPT_EXPOSE_BINS
 * uint64_t --, "expose_state" -- its device state record: a struct fovpt_expose_state --, "warp_keys" -- fovpt_warp's key
 * buffer, once made: the keys of the last warp in its first width * height uint64_t --, "focus_state" -- fovpt_focus's device
 * state record: a struct fovpt_focus_state --, "focus_scratch" -- its (r, tp) pairs, float2 per pixel, once made --,
 * "bloom_pyramid" -- fovpt_bloom's pyramid, once made: the levels of the last call, float4 texels packed one after the other --, ...) */
int fovpt_debug_buffer(fovpt_ctx* ctx, const char* name, void** ptr, size_t* bytes);

#ifdef __cplusplus
}
#endif

#ifdef __cplusplus
static_assert(sizeof(fovpt_material) == 104, "Material ABI");
static_assert(sizeof(fovpt_probe) == 64, "Probe ABI");
static_assert(sizeof(fovpt_launch_params) == 248, "LaunchParams ABI");
static_assert(sizeof(fovpt_denoise_config) == 32, "denoise config ABI");
static_assert(sizeof(fovpt_reconstruct_config) == 32, "reconstruct config ABI");
static_assert(sizeof(fovpt_gbuffer_ptrs) == 40, "gbuffer ABI");
static_assert(sizeof(fovpt_temporal_config) == 32, "temporal config ABI");
static_assert(sizeof(fovpt_post_config) == 112 && offsetof(fovpt_post_config, denoise) == 16 && offsetof(fovpt_post_config, reconstruct) == 48 &&
              offsetof(fovpt_post_config, temporal) == 80, "post config ABI");
static_assert(sizeof(fovpt_expose_config) == 80 && offsetof(fovpt_expose_config, low_permille) == 32 && offsetof(fovpt_expose_config, key) == 48,
              "expose config ABI");
static_assert(sizeof(struct fovpt_expose_state) == 32 && offsetof(struct fovpt_expose_state, weight_total) == 16, "expose state ABI");
static_assert(sizeof(fovpt_bloom_config) == 64 && offsetof(fovpt_bloom_config, exposure) == 16 && offsetof(fovpt_bloom_config, gain_fovea) == 28 &&
              offsetof(fovpt_bloom_config, _reserved) == 44, "bloom config ABI");
static_assert(sizeof(fovpt_warp_camera) == 48 && offsetof(fovpt_warp_camera, W) == 36, "warp camera ABI");
static_assert(sizeof(fovpt_warp_config) == 32 && offsetof(fovpt_warp_config, fill_radius) == 4, "warp config ABI");
static_assert(sizeof(struct fovpt_warp_counts) == 32 && offsetof(struct fovpt_warp_counts, direct) == 8, "warp counts ABI");
static_assert(sizeof(fovpt_warp_motion_config) == 32 && offsetof(fovpt_warp_motion_config, advance) == 8, "warp motion config ABI");
static_assert(sizeof(fovpt_focus_config) == 64 && offsetof(fovpt_focus_config, strength) == 16 && offsetof(fovpt_focus_config, _reserved) == 36,
              "focus config ABI");
static_assert(sizeof(struct fovpt_focus_state) == 32 && offsetof(struct fovpt_focus_state, count) == 16, "focus state ABI");
static_assert(sizeof(fovpt_lens_config) == 128 && offsetof(fovpt_lens_config, k) == 32 && offsetof(fovpt_lens_config, clip_r2) == 60 &&
              offsetof(fovpt_lens_config, border) == 80 && offsetof(fovpt_lens_config, _reserved) == 96, "lens config ABI");
static_assert(sizeof(fovpt_variance_config) == 32 && offsetof(fovpt_variance_config, depth_tolerance) == 12 &&
              offsetof(fovpt_variance_config, _reserved) == 20, "variance config ABI");
static_assert(sizeof(fovpt_variance_filter_config) == 48 && offsetof(fovpt_variance_filter_config, luminance_sigma) == 16 &&
              offsetof(fovpt_variance_filter_config, demodulate) == 28 && offsetof(fovpt_variance_filter_config, _reserved) == 32,
              "variance filter config ABI");
static_assert(sizeof(fovpt_quality_config) == 32 &&offsetof(fovpt_quality_config, _reserved) == 8, "quality config ABI");
static_assert(sizeof(fovpt_quality_sums) == 1344 && offsetof(fovpt_quality_sums, max_err) == 200 && offsetof(fovpt_quality_sums, windows) == 224 &&
              offsetof(fovpt_quality_sums, ring_pixels) == 304 && offsetof(fovpt_quality_sums, width) == 1328, "quality sums ABI");
static_assert(sizeof(fovpt_packet_pass) == 32 && offsetof(fovpt_packet_pass, texels) == 24, "packet pass ABI");
static_assert(sizeof(fovpt_packet_config) == 16 && offsetof(fovpt_packet_config, _reserved) == 12, "packet config ABI");
static_assert(sizeof(fovpt_packet_header) == 128 && offsetof(fovpt_packet_header, width) == 16 && offsetof(fovpt_packet_header, pass) == 32,
              "packet header ABI");
static_assert(sizeof(fovpt_vertex_update) == 16 && offsetof(fovpt_vertex_update, vertex) == 8, "vertex update ABI");
static_assert(sizeof(fovpt_mesh_transform) == 52 && offsetof(fovpt_mesh_transform, m) == 4, "mesh transform ABI");
static_assert(sizeof(fovpt_hierarchy_cost_info) == 32 && offsetof(fovpt_hierarchy_cost_info, updates) == 16, "hierarchy cost ABI");
static_assert(sizeof(fovpt_rebuild_info) == 64 && offsetof(fovpt_rebuild_info, requested) == 8 && offsetof(fovpt_rebuild_info, snapshot_update) == 48 &&
              offsetof(fovpt_rebuild_info, ms_build) == 56, "rebuild info ABI");
static_assert(sizeof(fovpt_mesh_skin) == 32 && offsetof(fovpt_mesh_skin, joints) == 16 && offsetof(fovpt_mesh_skin, weights) == 24, "mesh skin ABI");
static_assert(sizeof(fovpt_skin_pose) == 16 && offsetof(fovpt_skin_pose, matrices) == 8, "skin pose ABI");
static_assert(sizeof(fovpt_morph_target) == 24 && offsetof(fovpt_morph_target, index) == 8 && offsetof(fovpt_morph_target, delta) == 16, "morph target ABI");
static_assert(sizeof(fovpt_mesh_morph) == 24 && offsetof(fovpt_mesh_morph, targets) == 16, "mesh morph ABI");
static_assert(sizeof(fovpt_morph_pose) == 32 && offsetof(fovpt_morph_pose, weights) == 8 && offsetof(fovpt_morph_pose, num_joints) == 16 &&
              offsetof(fovpt_morph_pose, matrices) == 24, "morph pose ABI");
static_assert(sizeof(fovpt_packet_depth_config) == 16 && offsetof(fovpt_packet_depth_config, _reserved) == 4, "depth packet config ABI");
static_assert(sizeof(fovpt_packet_depth_header) == 192 && offsetof(fovpt_packet_depth_header, camera) == 128 &&
              offsetof(fovpt_packet_depth_header, near) == 176 && offsetof(fovpt_packet_depth_header, _reserved) == 180, "depth packet header ABI");
static_assert(offsetof(fovpt_launch_params, camera) == 104, "LaunchParams ABI");
static_assert(offsetof(fovpt_launch_params, traversable) == 160, "LaunchParams ABI");
static_assert(offsetof(fovpt_launch_params, probe) == 168, "LaunchParams ABI");
#endif

#endif /* FOVPT_H */
