// fovpt_device.h -- structures and launchers shared by the host API (fovpt_api.hip, api_post.hip, api_gather.hip), the BVH
// builder and refit (bvh_build.hip, refit.hip), the wavefront kernels (wavefront.hip), the traversal (traverse.hip) and the
// post-frame kernels.  gfx950 only.  The one compile-time switch is FOVPT_V_STEPSTAT (a diagnostic build, tools/build_variant.sh);
// everything else that can be set with -D is a numeric knob with its measured default.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/fovpt.h"
#include "fovpt_jobplan.h"      // FOVPT_BLOCK, FOVPT_MAX_PASSES, FOVPT_MAX_ITERS, FOVPT_SHARDS and the engine's other constants
#include "fovpt_animplan.h"     // RigChannel, RigWeights, MorphEntry: what the animation set-up lays out and rig.hip / refit.hip read

#define FOVPT_WAVE 64
#ifndef FOVPT_V_STEPSTAT
#define FOVPT_V_STEPSTAT 0         // 1: diagnostic build: k_traverse counts steps (tools/stepstat.py, raystat.py, stepcount.py, raytrace_dump.py)
#endif
#ifndef FOVPT_LEAF_MAX
#define FOVPT_LEAF_MAX 4          // triangles per BVH leaf (<= 8: three bits in the leaf code)
#endif
#define FOVPT_STACK 64            // traversal stack entries per ray, all in LDS (a wide node leaves <= 3 behind)
#define FOVPT_QUADS_PER_BLOCK (FOVPT_BLOCK / 4)
#ifndef FOVPT_TBLOCK
#define FOVPT_TBLOCK 64           // threads per block of k_traverse (64, 256 or 1024: the rays of a block share one LDS stack array).
                                  // 64 = a workgroup is ONE wave: it gives its slot, registers and 4.3 KB of LDS back the moment it ends (a
                                  // 256-thread block holds all four slots until its slowest wave is through), and with more workgroups than
                                  // slots the hardware's dispatcher is the run-time scheduler that atomics were too slow to be (EXPERIMENTS.md)
#endif
#define FOVPT_TQUADS (FOVPT_TBLOCK / 4)
#ifndef FOVPT_GRID_PER_CU
#define FOVPT_GRID_PER_CU 24        // closest-hit launches: 256-thread units per CU (8 = every wave slot once; 24 = three times as many
                                    // one-wave workgroups as slots, measured best of 8 / 16 / 24 / 32 / 64)
#endif
#ifndef FOVPT_GRID_SHADOW_PER_CU
#define FOVPT_GRID_SHADOW_PER_CU 6
#endif

// One triangle in BVH leaf order, pre-subtracted edges (exactly v1-v0 and v2-v0 in fp32,
// so Moeller-Trumbore gives the same bits as the contract in include/fovpt.h / oracle).
struct alignas(16) TriRec {
    float v0x, v0y, v0z, e1x;
    float e1y, e1z, e2x, e2y;
    float e2z;
    uint32_t prim;                // global primitive id (tie-break key)
    uint32_t mesh;
    uint32_t pad;
};                                // 48 B
static_assert(sizeof(TriRec) == 48, "TriRec");

// 4-wide BVH node: four 32-byte child records.  The traversal gives one ray to four adjacent lanes
// (a quad); lane j of the quad owns child j and fetches exactly its record (two 16-byte loads, the
// quad's eight loads cover the 128-byte node).  code >= 0: index of a wide node; code < 0: leaf,
// ~code = (offset of the first triangle in 16-byte units << 3) | (count-1).  An unused slot holds the degenerate box lo = hi = +inf,
// which no ray passes.
struct alignas(16) BvhChild {
    float lox, loy, loz, hix;
    float hiy, hiz;
    int32_t code;
    uint32_t pad;                 // 0..3, distinct within a node: where closest-hit rays rank this child among children they enter at the
                                  // same distance (the two lowest bits of the traversal's sort key; equal keys would collide on the stack)
};
struct alignas(16) BvhNode4 {
    BvhChild c[4];
};                                // 128 B
static_assert(sizeof(BvhNode4) == 128, "BvhNode4");

struct TexDev {
    const uint32_t* px;
    int32_t w, h;
};

struct MeshDev {                  // the SBT record of the reference (LaunchParams.h:38-47), minus geometry
    fovpt_material material;      // 104 B
    int32_t texture_id;           // <0: none
    int32_t has_texcoord;
    TexDev tex;                   // a copy of textures[texture_id]: one dependent load less on the way to the texels
};                                // 128 B

struct SceneView {
    const BvhNode4* nodes;
    const TriRec* tris;           // leaf order; lives in the nodes' allocation, tri_off bytes behind `nodes`
    const float2* tri_tc;         // 3 per global primitive id (or null)
    const MeshDev* meshes;
    const TexDev* textures;
    uint32_t num_tris;
    uint32_t any_catcher;
    uint32_t tri_off;             // (const char*)tris - (const char*)nodes: one base register reaches both
    uint32_t num_nodes;           // wide nodes of the hierarchy
};


struct PassDev {                  // one optixLaunch worth of parameters
    uint32_t gw, gh;              // launch grid
    uint32_t fx, fy, fz;          // frame.factor
    int32_t fill;                 // frame.fillSize
    uint32_t offx, offy;          // frame.offset
    float r_inner, r_outer;
    uint32_t spp;                 // samples_per_launch
    uint32_t subframe;            // frame.subframe_index
    uint32_t redraw;              // frame.redraw
    uint32_t slot_base;           // first sample slot of this pass
    uint32_t launch_base;         // first launch record of this pass
    uint32_t row0, row1;          // launch rows [row0, row1) handled by this job (a chunk of a large launch)
    uint32_t frame_pass;          // index of this launch within the caller's frame (P 0, M 1, F 2): the tile ownership of
                                  // launch_owned() rotates with it, also when the launch runs as a job of its own (chunks)
};

struct FrameDev {
    PassDev pass[FOVPT_MAX_PASSES];
    int32_t npass;
    int32_t w, h;                 // frame.size
    uint32_t cx, cy;              // frame.c
    float eye[3], U[3], V[3], W[3];
    fovpt_probe probe;            // device pointers
    const uint32_t* guide_x;      // lower_bound guide tables for probe.cdfValuesX / Y, or null
    const uint32_t* guide_y;
    const float4* probe_rec;      // packed {cdfX, pdfX, r, g, b} records per texel (two float4), or null
    int32_t probe_row_mul;        // 0 when all probe rows are identical (constant ambient probe), else 1
    fovpt_float4* accum;
    const fovpt_float4* accum_prev;   // what accumulate mode blends with: accum itself, or its copy from before a chunked launch
    uint32_t* frame;
    fovpt_float4 *g_normal, *g_color, *g_albedo;   // denoiser guide targets (null unless write_guides)
    uint32_t total_slots;
    int32_t max_depth;
    int32_t accumulate;
    int32_t rank, world, tile_w, tile_h;
    int32_t chunked;              // 1: this job is one of several over the same frame
    int32_t zero_holes;           // 1: clear the pixels no launch index of this job writes (a whole frame on a rank other than 0)
    int32_t options;              // fovpt_config.options (FOVPT_OPT_*): opt-in extensions, 0 = the reference's behaviour
    int32_t partition;            // 1: k_shade appends a block's next rays in two direction classes (foveated frames), see block_append2d
};

// Per-sample-slot path state (SoA, 16-B vectors so every access is one dwordx4).
// A radiance-ray queue holds the RAYS, not slot numbers: entry = origin.xyz + sample slot (bits of .w),
// direction.xyz.  Sharded like every queue (FOVPT_SHARDS regions of `cap` entries).  A traversal or shading
// wave reads 16 / 64 consecutive entries with coalesced loads and no indirection.
struct RayQueue {
    float4* o;
    float4* d;
};

struct PathState {
    float4* thr;        // pathThroughput.xyz, rayEta
    uint4* rng;         // Random.seed1, Random.seed2, stateFlags (DONE 1, SECONDARY 2, ALPHA_ONE 4) | depth << 8, unused
    float4* hit;        // t, u, v, tri position in leaf order as bits (0xffffffff = miss)
    float4* rad;        // [slot][depth]: prd.radiance of the segment at that depth (directLight = term 0,
                        // indirectLight = terms 1.. summed in order); one writer per cell
    size_t stride;      // cells per slot (= max_depth)
    float4* alpha;      // prd.alpha contribution of a shadow-catcher primary hit
    float4* guide_n;    // write_guides: prd.normal of the primary hit (deviceProgram.cu:509-512), else null
    float4* guide_a;    // write_guides: prd.albedo of the primary hit
    float4* backplate;  // per launch record: backplate of the last sample (deviceProgram.cu:495)
};

// Shadow (occlusion) ray queue, indexed by queue position.
struct ShadowQueue {
    float4* o;          // origin.xyz, slot as bits
    float4* d;          // direction.xyz, target as bits (depth cell of rad, or 0xffffffff = alpha)
    float4* val_vis;    // value added when NOT occluded
    float4* val_occ;    // value added when occluded
};

// Queues are sharded: shard s of a queue with capacity `cap` lives at [s*cap, s*cap + count[s]).
// One returning atomic on ONE word saturates at ~88/us on MI355X, so every producer block appends
// to the counter of shard blockIdx % 8 with one atomic per block-iteration.
// Queue sizes live per SHARD, each shard's block FOVPT_SHARD_STRIDE words away from the next: the blocks
// of one XCD append to one shard, and returning atomics on words of the same memory channel serialise
// (~88 per microsecond), so the eight shards must not share one.
#ifndef FOVPT_SHARD_STRIDE
#define FOVPT_SHARD_STRIDE 128    // uint32 words: 512 B (measured: 0.940 ms/frame; 4 KB: 0.957; all eight in one line: 0.977)
#endif
struct Counters {       // device-resident, zeroed per frame except the stats block
    uint32_t shard[FOVPT_SHARDS][FOVPT_SHARD_STRIDE];   // [s][it]: radiance queue size of iteration it (0 = camera rays);
                                                        // [s][FOVPT_MAX_ITERS + 1 + it]: shadow queue size
    unsigned long long stat_radiance, stat_shadow, stat_paths;
    // diagnostics of a -DFOVPT_V_STEPSTAT=1 build (tools/stepstat.py): per ray kind [closest, any-hit]
    // wave-level node steps, active quads in them, wave-level leaf steps, active quads in them
    unsigned long long diag[2][4];
};
static_assert(2 * (FOVPT_MAX_ITERS + 1) <= FOVPT_SHARD_STRIDE, "shard block holds both queues' sizes");
#define FOVPT_CNT_Q(it) (it)                               // word index inside a shard's block
#define FOVPT_CNT_SQ(it) (FOVPT_MAX_ITERS + 1 + (it))

// The padding of a triangle's box, ext its longest extent and mag its largest coordinate magnitude: the build's boxes
// (bvh_build.hip) and the refit's (refit.hip) are this one expression, so that every Moeller-Trumbore-accepted hit point lies
// well inside the box and the fused-multiply-add slab test of the traversal stays conservative.
__device__ inline float fovpt_tri_pad(float ext, float mag) { return 1e-4f * ext + 1e-5f * mag + 1e-20f; }

// ---- launchers implemented in wavefront.hip / traverse.hip / bvh_build.hip / refit.hip ----------------------
#define FOVPT_BVH_MAX_LEVELS 64   // levels of the wide tree recorded by the build (a traversable tree has at most (FOVPT_STACK - 1) / 3)
struct BvhBuildResult {
    BvhNode4* nodes;              // ONE allocation: the emitted nodes, then (256-byte aligned) the triangles; free `nodes` only
    TriRec* tris;
    uint32_t num_nodes;           // wide nodes emitted (breadth-first order, root = 0)
    uint32_t num_refs;            // triangle records behind the nodes: the triangles, or more when triangles were split into references
    uint32_t max_depth;
    uint32_t reinserted;          // 1: reinsertion rounds changed the PLOC tree
    size_t node_bytes, tri_bytes;
    uint32_t num_levels;          // levels of the wide tree (0: more than FOVPT_BVH_MAX_LEVELS)
    uint32_t level_first[FOVPT_BVH_MAX_LEVELS + 1];   // level L is the contiguous nodes [level_first[L], level_first[L + 1])
};
// a result nobody adopted: the allocation goes, br is left zeroed
inline void free_hierarchy(BvhBuildResult& br) { if (br.nodes) (void)hipFree(br.nodes); br = BvhBuildResult{}; }

// The environment switches of a build, read once by whoever asks for it (fovpt_bvh_switches), so that a build on a thread of its
// own never reads the environment: FOVPT_BVH (use_ploc), FOVPT_SPLIT (split_budget: references added by spatial splits as a
// fraction of the triangles, 0 = none, see bvh_build.hip), FOVPT_BVH_ORDER, FOVPT_REINSERT (rounds of reinsertion on the PLOC
// tree, 0 = none) and FOVPT_BVH_VERBOSE.
struct BvhSwitches { int use_ploc; float split_budget; int order_children, reinsert_rounds, verbose; };
BvhSwitches fovpt_bvh_switches();

// What every stage of a build left, for the test hook fovpt_debug_build (api_debug.hip): host copies of the build's own arrays,
// taken before the build moves on.  n = build primitives (references), ni = n - 1 internal nodes of the binary tree.  A tiny
// build (n <= FOVPT_LEAF_MAX) has no keys and no binary tree: only splits, boxes, bounds, vals_s, leaf_pos and nodes_pre.
struct BvhBuildTrace {
    int tiny = 0, splits = 0;                                 // splits: references were made (boxes come from k_split_emit)
    float s_cut = 0.f;                                        // the bisection's cut length (0: no split budget)
    std::vector<uint32_t> split_count, split_first, ref_prim; // per triangle (whenever the budget is on); per reference (splits only)
    std::vector<float> boxes;                                 // 6 per build primitive: lo.xyz, hi.xyz
    float cbounds[6] = {0, 0, 0, 0, 0, 0};                    // centroid bounds: min.xyz, max.xyz
    std::vector<uint64_t> keys_s;
    std::vector<uint32_t> vals_s;
    int root = 0;                                             // the binary tree as PLOC or Karras left it
    std::vector<int32_t> left0, right0;
    std::vector<float> ibox0;
    std::vector<uint32_t> round_end;                          // PLOC: internal nodes made up to and including each round
    std::vector<int32_t> left1, right1;                       // ... and as the collapse saw it (after reinsertion)
    std::vector<float> ibox1;
    std::vector<uint32_t> size_int, node_first, leaf_pos;
    std::vector<uint32_t> dp;                                 // 4 words per internal node: c1, c2, c3 (float bits), dec
    std::vector<uint32_t> nodes_pre;                          // the wide nodes before k_order_children, 32 words each
};

// flat: 9 floats per triangle (v0,v1,v2), mesh_of_prim: mesh id per triangle.  All device pointers.
// reinsert: rounds of reinsertion on the PLOC tree (0 = none, -1 = sw.reinsert_rounds).
// trace: null for every production build; set, each stage's arrays are copied to the host (a synchronisation per stage).
hipError_t fovpt_build_lbvh(hipStream_t st, const float* flat, const uint32_t* mesh_of_prim, uint32_t n, const BvhSwitches& sw,
                            int reinsert, BvhBuildResult* out, char* err, size_t errlen, BvhBuildTrace* trace = nullptr);

// cap = shard capacity (in items) of the radiance queues and of the shadow queue.
// sel: 0 = all eight queue shards (a whole job); 1 / 2 = the first / second four (one of the two chains of a frame)
// Returns the kernel it launched: 0 = k_generate, 1 = k_generate_owned.
int fovpt_launch_generate(hipStream_t st, const FrameDev& fd, PathState ps, RayQueue queue0, uint32_t cap, Counters* cnt, uint32_t slot_begin,
                          uint32_t slot_end, int grid, uint32_t sel = 0);
// One launch that traces the radiance queue of iteration it_closest (closest hit) OR the shadow queue of iteration
// it_shadow (occlusion): the other one is < 0 (traverse.hip).
void fovpt_launch_traverse(hipStream_t st, SceneView sc, PathState ps, RayQueue queue, ShadowQueue sq, uint32_t cap,
                           Counters* cnt, int it_closest, int it_shadow, int grid, hipEvent_t done = nullptr, uint32_t sel = 0);
void fovpt_launch_shade(hipStream_t st, const FrameDev& fd, SceneView sc, PathState ps, RayQueue queue_in, RayQueue queue_out,
                        ShadowQueue sq, uint32_t cap, Counters* cnt, int depth, int grid, hipEvent_t done = nullptr, uint32_t sel = 0);
void fovpt_launch_resolve(hipStream_t st, const FrameDev& fd, PathState ps, Counters* cnt, hipEvent_t done = nullptr);
// multi-GPU gather plan (see wavefront.hip): owner map + per-block counts; scan (phase 0) / fill (phase 1); pack; unpack
void fovpt_launch_plan_owner(hipStream_t st, const FrameDev& fd, uint8_t* owner, uint32_t* block_count, uint32_t nblocks);
void fovpt_launch_plan_scan_fill(hipStream_t st, uint32_t npix, uint32_t nblocks, int world, const uint8_t* owner, uint32_t* block_count,
                                 uint32_t* total, const uint32_t* rank_base, uint32_t* idx, int phase);
void fovpt_launch_gather_pack(hipStream_t st, uint32_t n, const uint32_t* idx, const uint32_t* frame, uint32_t* packed);
void fovpt_launch_gather_unpack(hipStream_t st, int world, uint32_t stride, uint32_t total, const uint32_t* base, const uint32_t* idx,
                                const uint32_t* gathered, uint32_t* frame);
// The post-frame kernels' tiling: one thread per pixel, a block a 64 x 4 pixel tile (a wave is 64 consecutive pixels of a row).
// fovpt_tile_grid: the grid that covers w x h; a thread finds its pixel with tile_pixel (fovpt_pixel.h).
#define FOVPT_TILE_W 64
#define FOVPT_TILE_H 4
static_assert(FOVPT_TILE_W == FOVPT_WAVE && FOVPT_TILE_W * FOVPT_TILE_H == FOVPT_BLOCK, "a wave per tile row, a block per tile");
inline dim3 fovpt_tile_grid(int w, int h) { return dim3((w + FOVPT_TILE_W - 1) / FOVPT_TILE_W, (h + FOVPT_TILE_H - 1) / FOVPT_TILE_H); }
// The launches of an a-trous filter after its prep kernel: iteration i reads the ping-pong buffer i & 1 and writes the other;
// step(i, last, in, out) launches it, `last` on the one that writes the outputs (fovpt_denoise, fovpt_variance_filter).
template <class Step>
inline void fovpt_atrous_iterate(int iterations, float4* b0, float4* b1, Step step)
{
    float4* buf[2] = {b0, b1};
    for (int i = 0; i < iterations; i++) step(i, i + 1 == iterations, buf[i & 1], buf[(i + 1) & 1]);
}
// fovpt_denoise (denoise.hip): level map + demodulation, then `iterations` a-trous launches (the last writes the outputs).
// I0 / I1: ping-pong float4 per pixel; level: one byte per pixel.
struct DenoiseArgs {
    int32_t n_pass[FOVPT_MAX_PASSES];   // iterations of the pixels whose last writer is pass p
    int32_t iterations;                 // max over the passes present
    float inv_c, inv_n, inv_a;          // 1 / sigma^2 (fp32, host)
};
void fovpt_launch_denoise(hipStream_t st, const FrameDev& fd, const DenoiseArgs& a, const fovpt_float4* color, const fovpt_float4* normal,
                          const fovpt_float4* albedo, float4* I0, float4* I1, uint8_t* level, fovpt_float4* out_color, uint32_t* out_rgba);
// fovpt_gbuffer / fovpt_reconstruct (reconstruct.hip).  The G-buffer: one camera ray per pixel of fd (jitter 0.5) into queue 0,
// all in shard 0 of cnt (k_gbuffer_rays); the caller traces them with fovpt_launch_traverse (closest hit, cap = w * h); then
// k_gbuffer_fill turns the hit records into the per-pixel outputs.
struct GBufferDev {
    uint32_t* prim;                     // global primitive id, 0xffffffff on a miss
    float4* pos;                        // eye + t * dir, t (miss: 0, 0, 0, -1)
    float4* nrm;                        // face-forwarded geometric normal, 0
    float4* alb;                        // material colour or texel, 0
};
void fovpt_launch_gbuffer_rays(hipStream_t st, const FrameDev& fd, RayQueue q, Counters* cnt);
void fovpt_launch_gbuffer_fill(hipStream_t st, const FrameDev& fd, SceneView sc, RayQueue q, const float4* hit, GBufferDev g);
struct ReconstructArgs {
    float inv_support[2];               // 1 / (support * f) for f = 2, 4 (fp32, host)
    float inv_n, inv_z;                 // 1 / sigma^2 of the normal and the depth term
    int32_t levels;                     // bit 0: fill-2 pixels, bit 1: fill-4 pixels
    int32_t remodulate;                 // 1: demodulate by the albedo guide, remodulate by the G-buffer's albedo
};
void fovpt_launch_reconstruct(hipStream_t st, const FrameDev& fd, const ReconstructArgs& a, const fovpt_float4* in, const fovpt_float4* albedo,
                              GBufferDev g, fovpt_float4* out_color, uint32_t* out_rgba);
struct TemporalArgs {
    float inv[9];                       // rows of the previous camera's inverse [U V W]^-1 (binary64 on the host, rounded to fp32)
    float eye_prev[3];                  // the previous camera's eye
    int32_t cap[4];                     // history caps: fill 1, fill 2, fill 4, FOV_OFF
    float normal_tol, depth_tol;        // |N_q - N_p|^2 <= normal_tol; |N_p . (X_q - X_p)| <= depth_tol * t_p
    int32_t reproject;                  // 0: no pixel reprojects (no previous step, or a singular previous camera)
    int32_t uniform;                    // the frame was rendered FOV_OFF
};
void fovpt_launch_temporal(hipStream_t st, const FrameDev& fd, const TemporalArgs& a, const fovpt_float4* in, GBufferDev g, GBufferDev gp,
                           const float4* hist_prev, float4* hist_out, fovpt_float4* out_color, uint32_t* out_rgba);
// fovpt_temporal_motion (temporal.hip, k_temporal_motion): what it reads beside k_temporal's inputs.  A hit pixel's mesh (the
// mesh of its triangle record, found through the hit record) has moved since the previous step when mark[mesh] == epoch; only
// then are tri_vidx, vtx_prev and the rest of the two records read.
struct TemporalMotionArgs {
    const float4* hit;                  // the G-buffer trace's hit records: t, u, v, record position in leaf order as bits
    const TriRec* tris;
    const uint64_t* mark;               // per mesh: the step (TemporalMotionArgs::epoch) before which it last moved
    const uint3* tri_vidx;              // per global primitive id its three vertices in vtx_prev (null until a mesh is marked)
    const float* vtx_prev;              // the positions marked meshes had at the previous step (null until a mesh is marked)
    fovpt_float4* out_motion;           // null: no motion vectors
    uint64_t epoch;                     // (64 bits: never wraps, so a stale mark never comes true again)
};
void fovpt_launch_temporal_motion(hipStream_t st, const FrameDev& fd, const TemporalArgs& a, const TemporalMotionArgs& m, const fovpt_float4* in,
                                  GBufferDev g, GBufferDev gp, const float4* hist_prev, float4* hist_out, fovpt_float4* out_color,
                                  uint32_t* out_rgba);
// fovpt_post with the reconstruction and the temporal step both on (post_fused.hip, k_reconstruct_temporal): fovpt_launch_reconstruct
// into registers, then fovpt_launch_temporal's step (m null) or fovpt_launch_temporal_motion's (m given) on that colour.  `in` and
// `albedo` are read across pixels: none of the written buffers may be one of them.
void fovpt_launch_reconstruct_temporal(hipStream_t st, const FrameDev& fd, const ReconstructArgs& ra, const TemporalArgs& ta,
                                       const TemporalMotionArgs* m, const fovpt_float4* in, const fovpt_float4* albedo, GBufferDev g,
                                       GBufferDev gp, const float4* hist_prev, float4* hist_out, fovpt_float4* out_color, uint32_t* out_rgba);
// fovpt_expose (expose.hip): the meter (AUTO: k_expose_meter into `rows`, one row of FOVPT_EXPOSE_BINS counts per block of
// fovpt_expose_rows(pixels); k_expose_adapt from them into the histogram and the state record), then the tone map (state null:
// at a.exposure).  ExposeState: the struct shares its name with the entry point, which hides it in C++.
typedef struct fovpt_expose_state ExposeState;
#define FOVPT_EXPOSE_BLOCK 1024          // threads per block of the meter and of k_expose_adapt
#ifndef FOVPT_EXPOSE_MAX_ROWS
#define FOVPT_EXPOSE_MAX_ROWS 512       // blocks of the meter: 2 per CU, every wave slot once; every row goes through the one block of k_expose_adapt
#endif
struct ExposeArgs {
    int32_t weight[4];                  // METER_GAZE: fill 1, fill 2, fill 4, FOV_OFF
    int32_t uniform;                    // the frame was rendered FOV_OFF
    int32_t low, high;                  // permille ranks of the trimmed mean
    float ev_min, ev_max, key, adapt_brighter, adapt_darker;
    int32_t tone;                       // FOVPT_TONE_*
    float white, exposure;              // REINHARD's white; FIXED's exposure
};
uint32_t fovpt_expose_rows(size_t npix);
void fovpt_launch_expose_meter(hipStream_t st, const FrameDev& fd, const ExposeArgs& a, bool gaze, const fovpt_float4* in, uint32_t* rows);
void fovpt_launch_expose_adapt(hipStream_t st, const ExposeArgs& a, const uint32_t* rows, uint32_t nrows, uint64_t* hist, ExposeState* state);
void fovpt_launch_expose_apply(hipStream_t st, size_t npix, const ExposeArgs& a, const ExposeState* state, const fovpt_float4* in,
                               fovpt_float4* out_color, uint32_t* out_rgba);
// fovpt_bloom (bloom.hip): the bright pass into level 0 of the pyramid (state: fovpt_expose's record where the exposure comes
// from it, else null), the levels down and back up, one launch each, then the composite.  pyramid: the levels packed one after
// the other (fovpt_bloom_level: the size of level k of a w x h frame and its first texel); it is none of the call's other buffers.
struct BloomArgs {
    int32_t flags;                      // FOVPT_BLOOM_*
    int32_t uniform;                    // the frame was rendered FOV_OFF
    float threshold, knee, exposure, intensity, spread;
    float gain[4];                      // GAINS: fill 1, fill 2, fill 4, FOV_OFF
};
void fovpt_bloom_level(int w, int h, int k, int* W, int* H, size_t* first);
void fovpt_launch_bloom(hipStream_t st, const FrameDev& fd, const BloomArgs& a, int levels, const ExposeState* state, const fovpt_float4* in,
                        float4* pyramid, fovpt_float4* out_color, uint32_t* out_rgba);
// fovpt_warp (warp.hip): the depth-tested scatter of fd's pixels (its camera: the directions of miss pixels) into `keys` -- one
// 64-bit key per pixel, all ones before the launch -- seen from the camera of a, then the resolve of the keys into the outputs.
// counts: FOVPT_WARP_COUNT_SLOTS copies of a struct fovpt_warp_counts on the device, FOVPT_WARP_COUNT_STRIDE 64-bit words apart
// (256 bytes: no two share a cache line), all zero before the scatter; a wave adds to the copy of its number, the sum over the
// copies is the record.  WarpCounts: the struct shares its name with the entry point, which hides it in C++.
typedef struct fovpt_warp_counts WarpCounts;
#define FOVPT_WARP_COUNT_SLOTS 256
#define FOVPT_WARP_COUNT_STRIDE 32
#define FOVPT_WARP_COUNT_BYTES ((size_t)FOVPT_WARP_COUNT_SLOTS * FOVPT_WARP_COUNT_STRIDE * sizeof(uint64_t))
struct WarpArgs {
    float inv[9];                       // rows of the `to` camera's inverse [U V W]^-1 (binary64 on the host, rounded to fp32)
    float eye[3];                       // the `to` camera's eye
};
void fovpt_launch_warp_scatter(hipStream_t st, const FrameDev& fd, const WarpArgs& a, const uint32_t* prim, const float4* pos, uint64_t* keys,
                               uint64_t* counts);
// fovpt_warp_motion (warp.hip, k_warp_scatter_motion): what its scatter reads beside k_warp_scatter's inputs -- fovpt_temporal_motion's
// per-pixel reads.  A hit pixel's mesh moved in the interval the last temporal step ended when mark[mesh] == epoch (that step's
// number); only then are tri_vidx and vtx_prev read, and the pixel scatters X* = X_s + advance * (X_s - X').  tri_bytes, num_prims
// and num_meshes bound what a hit record and a G-buffer entry may address: an entry outside them counts as not moved.
struct WarpMotionArgs {
    const float4* hit;                  // the last G-buffer trace's hit records: t, u, v, record position in 16-byte units as bits
    const TriRec* tris;
    const uint64_t* mark;               // per mesh: the step before which it last moved
    const uint3* tri_vidx;              // per global primitive id its three vertices in vtx_prev
    const float* vtx_prev;              // the positions the marked meshes had when the step before the last one ran
    uint64_t epoch;                     // the number of the last step
    uint64_t tri_bytes;                 // the triangle records' bytes
    uint32_t num_prims, num_meshes;
    float advance;
};
void fovpt_launch_warp_scatter_motion(hipStream_t st, const FrameDev& fd, const WarpArgs& a, const WarpMotionArgs& m, const uint32_t* prim,
                                      const float4* pos, uint64_t* keys, uint64_t* counts);
// fovpt_warp_depth (warp.hip, k_warp_scatter_depth): the scatter from a depth image (fd.w x fd.h floats: depth along W, +inf the
// sky) and the camera it was rendered with -- fd's size, eye, U, V and W; nothing else of fd is read
void fovpt_launch_warp_scatter_depth(hipStream_t st, const FrameDev& fd, const WarpArgs& a, const float* depth, uint64_t* keys, uint64_t* counts);
// in_color / out_color, in_rgba / out_rgba: both null where that image is not warped; out_map: may be null.  No output is an
// input or another output (a pixel reads other pixels' inputs)
void fovpt_launch_warp_resolve(hipStream_t st, int w, int h, int radius, const uint64_t* keys, const fovpt_float4* in_color, const uint32_t* in_rgba,
                               fovpt_float4* out_color, uint32_t* out_rgba, uint32_t* out_map, uint64_t* counts);
// fovpt_focus (focus.hip): the meter over the gaze disc's bounding square [x0, x1] x [y0, y1] (clipped to the frame on the host;
// x1 < x0 or y1 < y0: nothing to meter) with the rank search and the adapt step in its one block (AUTO), the per-pixel (r, tp)
// pairs into `rt` (state null: at a.inv_focus) and the gather.  No output of the gather is `in` or `rt` (a pixel reads other
// pixels').  FocusState: the struct shares its name with the entry point, which hides it in C++.
typedef struct fovpt_focus_state FocusState;
#define FOVPT_FOCUS_BLOCK 1024           // threads of the meter's one block
#define FOVPT_FOCUS_TILE_W 32            // outputs of a block of the gather: a thread each
#define FOVPT_FOCUS_TILE_H 16
struct FocusArgs {
    int32_t x0, x1, y0, y1;             // the meter's square
    int64_t cx, cy;                     // the rendered gaze
    int32_t meter_radius, rank_permille, max_radius;
    float strength, focus_default, adapt_nearer, adapt_farther;
    float inv_focus;                    // FIXED: 1.0f / focus_distance
};
void fovpt_launch_focus_meter(hipStream_t st, int w, const FocusArgs& a, const uint32_t* prim, const float4* pos, FocusState* state);
void fovpt_launch_focus_radius(hipStream_t st, size_t npix, const FocusArgs& a, const FocusState* state, const uint32_t* prim, const float4* pos,
                               float2* rt, float* out_coc);
void fovpt_launch_focus_gather(hipStream_t st, int w, int h, int max_radius, const fovpt_float4* in, const float2* rt, fovpt_float4* out_color,
                               uint32_t* out_rgba);
// fovpt_lens (lens.hip): the pre-distortion of `in` into the outputs.  `in` is neither output (a pixel reads other pixels').
struct LensArgs {
    float H[9];                         // reaim: rows of M [U_to V_to W_to], M the rendered camera's inverse (binary64 on the host, rounded to fp32)
    int32_t reaim;                      // a `to` camera was given
    int32_t filter, encode;             // FOVPT_LENS_*
    int32_t mono;                       // the three chroma factors have equal bits: one lookup serves the three channels
    float center[2], scale[2], k[4], chroma[3], clip_r2, src_center[2], src_scale[2], border[4];
};
void fovpt_launch_lens(hipStream_t st, int w, int h, const LensArgs& a, const fovpt_float4* in, fovpt_float4* out_color, uint32_t* out_rgba);
// fovpt_variance (variance.hip): one launch of k_variance_moments.  pos / nrm: the rendered frame's G-buffer; motion may be null;
// hist_prev is read only with has_history; out_variance is none of the inputs and neither history (a pixel reads other pixels').
struct VarianceArgs {
    float eye[3], m2[3];                // the rendered camera's eye and the third row of its inverse [U V W]^-1 (binary64 on the host, rounded to fp32)
    float depth_tol, normal_tol;
    int32_t cap, spatial_below, radius;
    int32_t has_history;                // a previous step of this frame size exists
};
void fovpt_launch_variance(hipStream_t st, const FrameDev& fd, const VarianceArgs& a, const fovpt_float4* in, const float4* pos, const float4* nrm,
                           const fovpt_float4* motion, const float4* hist_prev, float4* hist_out, fovpt_float4* out_variance);
// fovpt_variance_filter (variance.hip): level map + demodulation + the initial variance, then `iterations` a-trous launches (the
// last writes the outputs).  J0 / J1: ping-pong float4 per pixel (I, v); level: one byte per pixel (AtrousLevel, fovpt_post_pixel.h).
struct VFilterArgs {
    int32_t n_pass[FOVPT_MAX_PASSES];   // iterations of the pixels whose last writer is pass p
    int32_t iterations;                 // max over the passes present
    int32_t demodulate;
    float sl2, inv_n, inv_z;            // luminance_sigma^2, 1 / normal_sigma^2, 1 / depth_sigma^2 (fp32, host)
};
void fovpt_launch_vfilter(hipStream_t st, const FrameDev& fd, const VFilterArgs& a, const fovpt_float4* color, const fovpt_float4* variance,
                          GBufferDev g, float4* J0, float4* J1, uint8_t* level, fovpt_float4* out_color, uint32_t* out_rgba);
// fovpt_quality (quality.hip): k_quality_tile over the frame's 32 x 32 pixel tiles into `rows` -- one row of FOVPT_QUALITY_COLUMNS
// 64-bit partial sums per block of fovpt_quality_rows(w, h), a block striding over the tiles --, then the one block of
// k_quality_sum, which adds the columns (the maximum for max_err) and writes every byte of the record.  test and ref may be the
// same image; out_class may be null.
#define FOVPT_QUALITY_TILE 32            // pixels along a side of a tile
#define FOVPT_QUALITY_BLOCK 256          // threads of k_quality_tile: 4 pixels of the tile each
#define FOVPT_QUALITY_SUM_BLOCK 1024     // threads of k_quality_sum's one block
#define FOVPT_QUALITY_COLUMNS (8 * FOVPT_QUALITY_CLASSES + 2 * FOVPT_QUALITY_RINGS)
#ifndef FOVPT_QUALITY_MAX_ROWS
#define FOVPT_QUALITY_MAX_ROWS 1024      // blocks of k_quality_tile: 4 per CU; every row goes through the one block of k_quality_sum
#endif
struct QualityArgs {
    int64_t cx, cy;                     // the rendered gaze: (int64)(int32)frame.c
    int32_t flags, ring_width;
    int32_t uniform;                    // the frame was rendered FOV_OFF
};
uint32_t fovpt_quality_rows(int w, int h);
void fovpt_launch_quality(hipStream_t st, const FrameDev& fd, const QualityArgs& a, const uint32_t* test, const uint32_t* ref, uint64_t* rows,
                          fovpt_quality_sums* out_sums, uint8_t* out_class);
// fovpt_update_vertices (refit.hip).  vtx: the scene's vertex positions, xyz per vertex, all meshes one after the other;
// tri_vidx: per global primitive id the three indices of its vertices in vtx.
#define FOVPT_GATHER_BATCH 32
struct VertexGather {                   // up to FOVPT_GATHER_BATCH device arrays of xyz triples, each copied into vtx at dst
    const float* src[FOVPT_GATHER_BATCH];
    uint32_t dst[FOVPT_GATHER_BATCH];   // first vertex in vtx
    uint32_t n[FOVPT_GATHER_BATCH];     // vertices
    int32_t count;
    uint32_t max_n;
};
void fovpt_launch_gather_vertices(hipStream_t st, const VertexGather& g, float* vtx);
// the copy-on-first-write of fovpt_temporal_motion's tracking: the batch's meshes (src: their positions in vtx) into vtx_prev,
// and mark[mesh[u]] = epoch
struct VertexTrack {
    uint32_t first[FOVPT_GATHER_BATCH]; // first vertex in vtx and vtx_prev
    uint32_t n[FOVPT_GATHER_BATCH];     // vertices
    uint32_t mesh[FOVPT_GATHER_BATCH];
    int32_t count;
    uint32_t max_n;
};
void fovpt_launch_gather_vertices_prev(hipStream_t st, const VertexTrack& g, const float* vtx, float* vtx_prev, uint64_t* mark, uint64_t epoch);
// fovpt_update_transforms: up to FOVPT_GATHER_BATCH meshes, each the n vertices from `first` on of rest through its row-major
// 3 x 4 matrix into vtx (x' = ((m0 x + m1 y) + m2 z) + m3, unfused binary32)
struct VertexTransform {
    float m[FOVPT_GATHER_BATCH][12];
    uint32_t first[FOVPT_GATHER_BATCH]; // first vertex in rest and vtx
    uint32_t n[FOVPT_GATHER_BATCH];     // vertices
    int32_t count;
    uint32_t max_n;
};
void fovpt_launch_transform_vertices(hipStream_t st, const VertexTransform& g, const float* rest, float* vtx);
// fovpt_update_animated's rigid bindings: VertexTransform with the matrices in device memory (k_rig_pose wrote them)
struct VertexTransformDev {
    const float* m[FOVPT_GATHER_BATCH]; // 12 floats each
    uint32_t first[FOVPT_GATHER_BATCH]; // first vertex in rest and vtx
    uint32_t n[FOVPT_GATHER_BATCH];     // vertices
    int32_t count;
    uint32_t max_n;
};
void fovpt_launch_transform_vertices_dev(hipStream_t st, const VertexTransformDev& g, const float* rest, float* vtx);
// fovpt_update_animated (rig.hip): one clip of a rig sampled at `time`, the nodes' world matrices composed level by level, and from
// them the palettes of the bound skinned meshes (into their places in skin_pal), the matrices of the rigid bindings and the
// weights of the bound morphed meshes (into their places in morph_w).  One workgroup of `threads` (a multiple of 64, at least
// num_nodes, at most FOVPT_RIG_MAX_NODES).  The definition is include/fovpt.h's, operation by operation.
// (RigChannel, RigWeights: fovpt_animplan.h, which lays them out)
struct RigDev {
    uint32_t num_nodes, num_levels, num_pal, num_rigid, num_wjobs;
    const int32_t* parent;          // per node
    const uint32_t* level;          // per node: 0 for a root, its parent's + 1 otherwise
    const float* rest;              // per node 10 floats: translation, rotation, scale
    const int32_t* node_chan;       // the clip's: per node the channels of its translation, rotation and scale (-1: rest)
    const int32_t* w_chan;          // the clip's: per RigWeights its channel (-1: zeros)
    const RigChannel* chan;
    const float* times;
    const float* values;
    const uint32_t* pal_node;       // per palette entry (the joints of the bindings, in binding order) its node,
    const uint32_t* pal_dst;        // its joint's place in skin_pal
    const float* inv_bind;          // and its inverse bind matrix, 12 floats
    const uint32_t* rigid_node;     // per rigid binding its node
    const RigWeights* wjobs;
    float* skin_pal;
    float* morph_w;
    float* world;                   // out: num_nodes x 12
    float* rigid;                   // out: num_rigid x 12
    float* palette;                 // out: num_pal x 12, what went to skin_pal, in binding order
};
void fovpt_launch_rig_pose(hipStream_t st, const RigDev& r, float time, uint32_t threads);
// fovpt_update_skinned: up to FOVPT_GATHER_BATCH meshes, each the n vertices from `first` on of rest through the blend of its
// four joints' matrices into vtx (M[e] = ((w0 J[j0][e] + w1 J[j1][e]) + w2 J[j2][e]) + w3 J[j3][e], then VertexTransform's
// expression with M; unfused binary32).  Vertex i of mesh u has its four joint indices at joints[skin[u] + i] and its weights at
// weights[skin[u] + i]; pal[u] is the mesh's palette, 12 floats per joint.
struct VertexSkin {
    const float* pal[FOVPT_GATHER_BATCH];
    uint32_t first[FOVPT_GATHER_BATCH]; // first vertex in rest and vtx
    uint32_t n[FOVPT_GATHER_BATCH];     // vertices
    uint32_t skin[FOVPT_GATHER_BATCH];  // first vertex in joints and weights
    int32_t count;
    uint32_t max_n;
};
void fovpt_launch_skin_vertices(hipStream_t st, const VertexSkin& g, const float* rest, const uint2* joints, const float4* weights, float* vtx);
// fovpt_update_morphed: up to FOVPT_GATHER_BATCH meshes, each the n vertices from `first` on of rest through their morph entries
// into vtx.  Vertex i of mesh u has the entries ent[off[o + i]] .. ent[off[o + i + 1]), o = this->off[u], sorted by target; an
// entry {dx, dy, dz, target} whose weight w[u][target] is not zero adds w * d to the position (unfused binary32, ascending
// targets).  pal[u], in a batch given to fovpt_launch_morph_skin_vertices, is the mesh's palette and skin[u] its first vertex
// in joints and weights: the morphed position then goes through VertexSkin's expression.
// (MorphEntry {dx, dy, dz, target}, 16 bytes: fovpt_animplan.h)
struct VertexMorph {
    const float* w[FOVPT_GATHER_BATCH];     // the mesh's weights, one per target
    const float* pal[FOVPT_GATHER_BATCH];   // (morph and skin only)
    uint32_t first[FOVPT_GATHER_BATCH];     // first vertex in rest and vtx
    uint32_t n[FOVPT_GATHER_BATCH];         // vertices
    uint32_t off[FOVPT_GATHER_BATCH];       // the mesh's first offset in morph_off (n + 1 of them)
    uint32_t skin[FOVPT_GATHER_BATCH];      // (morph and skin only)
    int32_t count;
    uint32_t max_n;
};
void fovpt_launch_morph_vertices(hipStream_t st, const VertexMorph& g, const float* rest, const uint32_t* off, const MorphEntry* ent, float* vtx);
void fovpt_launch_morph_skin_vertices(hipStream_t st, const VertexMorph& g, const float* rest, const uint32_t* off, const MorphEntry* ent,
                                      const uint2* joints, const float4* weights, float* vtx);
// fovpt_hierarchy_cost: the SAH cost of the num_nodes wide nodes in binary64, the same value from run to run.  partial: two
// doubles per block of fovpt_tree_cost_blocks(num_nodes); rec: where the result goes (device-visible memory).
struct TreeCostRecord { double cost, root, node, leaf; };     // (root + node + 2.7 leaf) / root and its three terms
inline uint32_t fovpt_tree_cost_blocks(uint32_t num_nodes) { return (uint32_t)((4ull * num_nodes + FOVPT_BLOCK - 1) / FOVPT_BLOCK); }
void fovpt_launch_tree_cost(hipStream_t st, const BvhNode4* nodes, uint32_t num_nodes, double* partial, TreeCostRecord* rec);
// one launch per level of the wide tree, deepest first (levels[0 .. num_levels]: level_first of the build)
void fovpt_launch_refit(hipStream_t st, BvhNode4* nodes, TriRec* tris, const uint32_t* levels, uint32_t num_levels, const uint3* tri_vidx,
                        const float* vtx);
// the build's input over the current vertices: 9 floats per primitive (v0, v1, v2)
void fovpt_launch_flatten(hipStream_t st, uint32_t n, const uint3* tri_vidx, const float* vtx, float* flat);
void fovpt_launch_build_guide(hipStream_t st, const float* cdf, int n, int segments, uint32_t* guide);
void fovpt_launch_probe_records(hipStream_t st, size_t n, const float* cdfX, const float* pdfX, const float4* data, float4* rec);
void fovpt_launch_build_cdf(hipStream_t st, int w, int h, const float4* data, float* pdfX, float* cdfX, float* pdfY, float* cdfY, float* row_total);
void fovpt_launch_math(hipStream_t st, int op, const float* a, const float* b, float* out, size_t n);
// shade_debug.hip: the device functions of a shaded hit (fovpt_shade_fn.h, tex2d) on n chosen inputs, one thread each
void fovpt_launch_debug_probe_sample(hipStream_t st, const fovpt_probe& pr, const uint32_t* guide_x, const uint32_t* guide_y, const float4* rec, int row_mul,
                                     int n, const float2* r12, int2* rowcol, float* out7);
void fovpt_launch_debug_probe_eval(hipStream_t st, const fovpt_probe& pr, int row_mul, int n, const float* dir3, float* out6);
void fovpt_launch_debug_bsdf(hipStream_t st, const fovpt_material& mat, int n, const float* in16, float* out16);
void fovpt_launch_debug_tex2d(hipStream_t st, const TexDev* textures, int texture, int n, const float2* uv, float4* out);
