// fovpt_ctx.h -- private to the host half of libfovpt (fovpt_api.hip, api_animate.hip, api_post.hip, api_view.hip, api_gather.hip,
// api_packet.hip, api_debug.hip): the context, the buffers it owns, and the helpers more than one of those files uses.  The
// frame engine's state is grouped (fovpt_ctx::engine: lanes, state sets, rotation, grids, knobs, timing events), and so is the
// post-frame stages': the record of the rendered frame (fovpt_ctx::rendered) and one struct per stage.  Host only: no kernel file
// includes it.
#pragma once
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "fovpt_bgjob.h"
#include "fovpt_device.h"
#include "fovpt_jobplan.h"      // the engine's constants and decisions (plan_job, chunk_rows, shard_capacity, chain_split)
#include <rccl/rccl.h>      // types only: the library is loaded at run time (fovpt_comm_*), libfovpt.so does not link it

// Device memory with one owner: freed by release(), by a growing reserve() and when the holder goes away.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    hipError_t reserve(size_t n)
    {
        if (n <= bytes) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; bytes = 0;
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    void swap(DevBuf& o) { void* q = p; p = o.p; o.p = q; const size_t n = bytes; bytes = o.bytes; o.bytes = n; }
};

#define FOVPT_LOCAL __attribute__((visibility("hidden")))      // a type whose members the library does not export

// A post-frame stage's own outputs: a float4 colour and an rgba8 image per pixel.
struct FOVPT_LOCAL OutPair {
    DevBuf color, rgba;
    hipError_t reserve(size_t n) { const hipError_t e = color.reserve(n * 16); return e != hipSuccess ? e : rgba.reserve(n * 4); }   // both, for n pixels
};

enum TimedKind { T_GENERATE, T_TRACE, T_SHADE, T_SHADOW, T_RESOLVE };    // what a timed launch adds to in fovpt_stats
struct EventPair { hipEvent_t a, b; TimedKind kind; };

// The completion events of one chain's shading and occlusion launches, per iteration
struct ChainEvents { hipEvent_t shade[FOVPT_MAX_ITERS + 1], shadow[FOVPT_MAX_ITERS + 1]; };

struct StateSet {
    DevBuf s_thr, s_rng, s_hit, s_rad, s_alpha, s_backplate, s_guide_n, s_guide_a;
    DevBuf q_o[2], q_d[2], counters;       // q_*: the two radiance-ray queues (ping-pong)
    DevBuf sq_o[FOVPT_NSQ], sq_d[FOVPT_NSQ], sq_vis[FOVPT_NSQ], sq_occ[FOVPT_NSQ];   // shadow queues, one per bounce in flight
    ChainEvents chain[2] = {};             // [1]: the second chain of a frame (fovpt_config.chains_per_frame = 2)
    hipEvent_t ev_done = nullptr;          // recorded after the resolve of the last job that used this set
    bool used = false;
};

// The frame engine (run_passes / run_job, fovpt_api.hip): everything a job is issued with.  Filled by fovpt_create (make_engine),
// which reads the environment switches once.
struct FOVPT_LOCAL Engine {
    // Second LANE (round 3): consecutive jobs alternate between two (main, shadow) stream pairs, so the main chain of job k+1
    // -- generate, closest-hit, shade, strictly one after the other -- runs BESIDE the main chain of job k instead of behind it:
    // the launch gaps, ramps and tails of one chain are filled by the other.  Resolves stay in job order (each waits for the
    // previous job's), and `shadow_stream` remains the one stream every finished frame is ordered on (fovpt_stream()).
    hipStream_t lane_main[FOVPT_MAX_LANES] = {}, lane_shadow[FOVPT_MAX_LANES] = {};   // [0] = the context's stream / shadow_stream
    // Every stream beside shadow_stream that may trace the scene or read its triangle records: the lanes' main streams and the
    // later lanes' shadow streams, once each, in lane order.  Whoever waits for, or records behind, "everything that traces"
    // walks these and names shadow_stream itself: first or last, as its order asks.
    hipStream_t trace_stream[2 * FOVPT_MAX_LANES - 1] = {};
    int num_trace_streams = 0;
    // Wavefront state, several sets used in rotation by consecutive jobs: the tail of job k (its last occlusion
    // rays and its resolve, on the shadow stream) runs beside the head of job k+1 (generate, camera rays).
    // Round 4: TWICE as many sets as lanes, so that the job which follows job k on the same lane (job k + lanes) does not
    // wait for job k's resolve before it may overwrite the path state: its main chain starts as soon as job k's has ended,
    // and k's tail runs beside it.  (What a 1/N shard of a frame needs: its launches are short, and last occlusion launch +
    // resolve were a third of a lane's cycle.)
    StateSet set[2 * FOVPT_MAX_LANES];
    PlanKnobs knobs;                       // lanes, nsets, chains_default, spread_occlusion (fovpt_jobplan.h)
    PlanRotation rot;                      // jobs issued so far and the set the last one used
    int grid = 2048, grid_trace = 2048, grid_shadow = 1024, grid_shade = 1024;   // blocks of generate, closest-hit, occlusion and shading launches
    uint64_t slot_budget = 64ull << 20;    // sample slots per wavefront job (~330 B of state and queues each and per set; jobs above FOVPT_SETS_SLOT_LIMIT rotate through one set per lane)
    DevBuf accum_before;                   // accumulate mode, chunked launch: the accum buffer as it was before the pass
    bool refit_pending = false;            // a refit has recorded fovpt_ctx::ev_scene since the last job: the trace streams wait for it, once
    std::vector<EventPair> pending;        // profile: the timed launches not yet read (drain_events), and events free for reuse
    std::vector<hipEvent_t> free_events;
};

struct fovpt_ctx {
    int device = 0;
    int num_cus = 256;
    hipStream_t stream = nullptr;          // main chain: generate, closest-hit traversal, shade
    hipStream_t shadow_stream = nullptr;   // occlusion rays of every bounce and the resolve: off the critical path
    Engine engine;                         // the frame engine: lanes, state sets, rotation, grids, knobs, timing events
    std::string err;
    fovpt_config cfg;
    // scene
    bool has_scene = false;
    uint64_t scene_id = 0;
    BvhNode4* nodes = nullptr;
    TriRec* tris = nullptr;
    DevBuf tri_tc, meshes, textures;
    std::vector<void*> tex_pixels;
    uint32_t num_tris = 0, any_catcher = 0;
    uint32_t bvh_levels[FOVPT_BVH_MAX_LEVELS + 1] = {};   // the wide tree's levels (BvhBuildResult::level_first), for the refit
    uint32_t bvh_num_levels = 0;
    // fovpt_update_vertices.  What fovpt_set_scene keeps on the host: per mesh its first global primitive, first vertex in the
    // concatenated vertex array and vertex count; per primitive the indices of its three vertices in that array; the positions.
    // Made on the first update: their device copies (up_vtx 12 B per vertex, up_vidx 12 B per primitive), two pinned staging
    // buffers for host updates used in turn (each reused once its previous copy has run: ev), and the event a refit records on
    // fovpt_stream(), which every lane stream waits for before the next job traces the scene (engine.refit_pending).
    std::vector<uint32_t> mesh_prim0, mesh_vbase, mesh_nv, h_tri_vidx;
    std::vector<float> h_vtx;
    DevBuf up_vtx, up_vidx;
    struct Staging { void* p = nullptr; size_t bytes = 0; hipEvent_t ev = nullptr; bool pending = false; } up_stage[2];
    int up_next = 0;
    hipEvent_t ev_scene = nullptr;
    // fovpt_update_transforms.  Made on a scene's first call and dropped by fovpt_set_scene: the device copy of h_vtx (12 B per
    // vertex) and, per mesh, the largest |coordinate| of its rest positions (the overflow rule)
    DevBuf rest_vtx;
    std::vector<double> mesh_absmax;
    // fovpt_set_skins / fovpt_update_skinned.  skins: empty until a scene's first fovpt_set_skins, then one entry per mesh
    // (num_joints 0: no skin) with the host copy of the skin, its largest weight sum S (the overflow rule), the mesh's first
    // vertex in skin_joints / skin_weights (the skinned meshes' vertices in mesh order: 8 B of indices and 16 B of weights each)
    // and its first joint in skin_pal (12 floats per joint, where host matrices go; rest_vtx and up_stage are shared with the
    // calls above).  Laid out anew by every fovpt_set_skins (fovpt_animplan.h, plan_skins: the rules, S and the places); dropped by
    // fovpt_set_scene.
    struct Skin { uint32_t num_joints = 0, first = 0, pal_first = 0; double S = 0.0; std::vector<uint16_t> joints; std::vector<float> weights; };
    std::vector<Skin> skins;
    DevBuf skin_joints, skin_weights, skin_pal;
    // fovpt_set_morphs / fovpt_update_morphed.  morphs: empty until a scene's first fovpt_set_morphs, then one entry per mesh
    // (num_targets 0: no morphs) with the host copy of the targets transposed into a per-vertex list -- off: num_vertices + 1
    // offsets into ent, relative to the mesh's first entry; ent: 16-byte records {dx, dy, dz, target}, sorted by target within
    // a vertex --, D[t] the largest |delta component| of target t (the overflow rule), the mesh's first offset in morph_off
    // (the morphed meshes in mesh order, num_vertices + 1 each, absolute into morph_ent), its first entry in morph_ent and its
    // first weight in morph_w (where host weights go).  Laid out anew by every fovpt_set_morphs (fovpt_animplan.h, plan_morphs: the
    // rules, the transposition, D and the places); dropped by fovpt_set_scene.
    struct Morph { uint32_t num_targets = 0, off_first = 0, ent_first = 0, w_first = 0; std::vector<double> D; std::vector<uint32_t> off; std::vector<MorphEntry> ent; };
    std::vector<Morph> morphs;
    DevBuf morph_off, morph_ent, morph_w;
    // fovpt_set_rig / fovpt_update_animated.  rig.set: a rig is there (made by fovpt_set_rig; dropped by a later fovpt_set_skins,
    // fovpt_set_morphs, fovpt_set_scene or fovpt_set_rig(NULL)).  bound: the bindings in their order, each with what its mesh goes
    // through and its place among the rigid matrices.  in: everything k_rig_pose reads, one allocation (the nodes' parents,
    // levels and rest poses, per clip the nodes' channel table and the weights' channels, the channels, key times and key values,
    // and per palette entry its node, its place in skin_pal and its inverse bind matrix); out: what it writes beside skin_pal and
    // morph_w (the worlds, the rigid matrices and the palettes in binding order: fovpt_debug_buffer "rig_world", "rig_rigid",
    // "rig_palette").  dev: the kernel's arguments, node_chan / w_chan those of clip 0 (a clip's tables follow its predecessor's).
    // The rules, the sections of `in` and the thread count are fovpt_animplan.h's (plan_rig), and so is RigBound.
    using RigBound = ::RigBound;
    struct Rig {
        bool set = false;
        uint32_t num_clips = 0, threads = 64;
        std::vector<RigBound> bound;
        DevBuf in, out;
        RigDev dev{};
    } rig;
    // fovpt_hierarchy_cost.  cost_built / cost_current / cost_updates / cost_measured: the caller's record.  cost_partial: the
    // block sums of k_tree_cost, sized when a hierarchy is adopted.  cost_slot: result records in pinned host memory the final
    // kernel writes, each with the event recorded behind it and the update number it measures; a slot is free once its event has
    // completed and its value is taken (take_costs).  cost_watching: a refit is followed by a measurement.
    struct CostSlot { TreeCostRecord* rec = nullptr; hipEvent_t ev = nullptr; bool pending = false; uint64_t update = 0; } cost_slot[4];
    DevBuf cost_partial;
    bool cost_watching = false;
    double cost_built = 0.0, cost_current = 0.0;
    uint64_t cost_updates = 0, cost_measured = 0;
    // FOVPT_UPDATE_REBUILD_ASYNC (api_animate.hip).  rb: made by a context's first flagged call, with the builder's stream (lowest
    // priority), the snapshot's event and the pinned record its cost measurement writes; a context that never passes the flag
    // has none of it.  The builder's thread (fovpt_bgjob.h) touches nothing of the context but *rb's `in` members, which the
    // requesting call fills before the thread starts and nobody else reads while it runs, and the RebuildDone it publishes:
    // the hierarchy, its cost, and the partial sums the measurement used, sized for that hierarchy (they become cost_partial).
    // flat / mesh_of: the snapshot (36 + 4 bytes per triangle), kept until the scene goes.  retired: hierarchies (and their
    // partial sums) that frames issued before an adoption may still read, each with events recorded behind everything that can;
    // freed once a poll finds them all complete (retire_poll), or when the device is idle.
    struct RebuildDone { BvhBuildResult br{}; float ms = 0.f; double cost = 0.0; void* partial = nullptr; size_t partial_bytes = 0; };
    struct Rebuild {
        fovpt::BgJob<RebuildDone> job;
        hipStream_t st = nullptr;
        hipEvent_t ev_snapshot = nullptr;
        TreeCostRecord* rec = nullptr;
        DevBuf flat, mesh_of;
        struct In { int device = 0; uint32_t ntri = 0; std::vector<uint32_t> h_mesh_of; BvhSwitches sw{}; int delay_ms = 0; } in;
        uint64_t snapshot_update = 0;
        double ms_build = 0.0;                 // of the last build that finished and has left the slot (one that waits there has its own)
        uint64_t failed_told = 0;              // the failed builds whose text fovpt_rebuild_state has given
        ~Rebuild();
    };
    std::unique_ptr<Rebuild> rb;
    struct Retired { void* p[2]; std::vector<hipEvent_t> ev; };
    std::vector<Retired> retired;
    // probe
    DevBuf pr_data, pr_pdfx, pr_cdfx, pr_pdfy, pr_cdfy, pr_guidex, pr_guidey, pr_rec;
    bool guide_ok = false;
    int guide_w = 0, guide_h = 0;
    bool rows_identical = false;           // every row of data / pdfX / cdfX equals row 0 bit for bit
    // frame buffers (resize)
    DevBuf fb_frame, fb_accum, fb_color, fb_normal, fb_albedo;
    // multi-GPU gather plan (fovpt_gather_plan): pixel indices grouped by owning rank
    DevBuf plan_owner, plan_blocks, plan_total, plan_base, plan_idx;
    std::vector<uint32_t> plan_off;        // host copy: rank r owns plan_idx[plan_off[r] .. plan_off[r + 1])
    std::string plan_key;                  // what the plan was built for
    // ---- the post-frame stages (api_post.hip, api_view.hip): the record of the rendered frame they all read, then one struct per
    // stage with what that stage owns, `out` being its own outputs.  post_resize keeps what exists of them at the frame's size.
    // The frame last issued with fovpt_render as it was rendered (w x h; 0 x 0: none since create / resize): its passes, gaze
    // and camera (frame), and the FOV_OFF flag, guides and shard count of its config.  Post-processing, the packet encoder and
    // the quality metric read these, never the caller's current config, gaze or camera.  Set by fovpt_render, cleared by
    // post_resize, and by nothing else.
    struct FOVPT_LOCAL Rendered {
        int w = 0, h = 0;
        FrameDev frame{};
        int32_t uniform = 0, guides = 0, world = 1;
        size_t pixels() const { return (size_t)w * (size_t)h; }
    } rendered;
    // fovpt_denoise: the level map, the ping-pong filter buffers and the context's own outputs (allocated on first use)
    struct FOVPT_LOCAL Denoise { DevBuf level, i0, i1; OutPair out; } denoise;
    // fovpt_gbuffer / fovpt_reconstruct: the G-buffer's own ray queue, hit records, counters and outputs (never a render state
    // set: a frame in flight may be using those); all allocated on first use.  pixels: the pixels of the last G-buffer trace
    // (fovpt_debug_buffer "gbuffer_hit")
    struct FOVPT_LOCAL GBuffer { DevBuf o, d, hit, cnt, prim, pos, nrm, alb; size_t pixels = 0; } gbuffer;
    // fovpt_reconstruct, fovpt_post (the chain's last stage) and fovpt_lens: the context's own outputs, allocated on first use
    // (the stages keep nothing else; everything else the chain uses is the stages' own: the denoiser's buffers, the temporal
    // step's sets, histories and state)
    struct FOVPT_LOCAL OwnOutputs { OutPair out; } reconstruct, post, lens;
    // fovpt_temporal: two G-buffer sets and two histories (rgb, n), used in turn by consecutive calls (last: the set the
    // last call wrote), the previous step's camera and size, and the context's own outputs; all allocated on first use.
    // valid: a previous step exists (dropped by fovpt_temporal_reset, fovpt_resize and fovpt_set_scene)
    struct FOVPT_LOCAL Temporal {
        DevBuf prim[2], pos[2], nrm[2], alb[2], hist[2];
        OutPair out;
        int last = 0, w = 0, h = 0;
        bool valid = false;
        float eye[3] = {}, U[3] = {}, V[3] = {}, W[3] = {};
    } temporal;
    // fovpt_temporal_motion: tracking of the positions meshes had at the previous temporal step.  Switched on by a context's
    // first fovpt_temporal_motion (tm_tracking; off again after fovpt_set_scene), which makes tm_mark: per mesh the number of the
    // step (tm_epoch, counted over both entry points) before which fovpt_update_vertices last moved it, 0 = never; the host's
    // copy is tm_mesh_epoch.  A mesh has moved since the previous step when its mark equals tm_epoch, so ending an interval is
    // tm_epoch++ on the host and nothing on the device.  vtx_prev (12 B per vertex, made by the first tracked update) holds, for
    // the marked meshes, what up_vtx held before the interval's first update of them.  tm_untracked: an update ran since the
    // previous step while tracking was off (the next fovpt_temporal_motion step has no history).
    bool tm_tracking = false, tm_untracked = false;
    uint64_t tm_epoch = 1;                 // (64 bits: never wraps)
    std::vector<uint64_t> tm_mesh_epoch;
    DevBuf tm_mark, vtx_prev;
    // fovpt_expose: the device state record (a struct fovpt_expose_state, zeroed when made and by a reset: steps 0 = the next
    // AUTO step is a first step; the host never reads it outside fovpt_expose_state), the meter's per-block histogram rows and
    // the histogram of the last metered step, and the context's own outputs; all allocated on first use
    struct FOVPT_LOCAL Expose { DevBuf state, rows, hist; OutPair out; } expose;
    // fovpt_bloom: the pyramid (float4 texels, the levels packed one after the other; texels: those of the last call's levels,
    // fovpt_debug_buffer "bloom_pyramid") and the context's own outputs; all allocated on first use
    struct FOVPT_LOCAL Bloom { DevBuf pyramid; size_t texels = 0; OutPair out; } bloom;
    // fovpt_warp: the scatter's keys (8 bytes per pixel), the device counts (FOVPT_WARP_COUNT_SLOTS partial records, zeroed on the stream
    // ahead of every warp; the host reads and adds them nowhere but in fovpt_warp_counts) and the context's own outputs; all allocated on
    // first use
    // depth_keys: fovpt_warp_depth's own keys, for the size of its last call (grown on demand; not the rendered frame's, so a
    // resize leaves them alone); the counts record is the one of all three kinds of warp
    struct FOVPT_LOCAL Warp { DevBuf keys, counts, depth_keys; OutPair out; } warp;
    // fovpt_focus: the device state record (a struct fovpt_focus_state, zeroed when made and by a reset: steps 0 = the next AUTO
    // step is a first step; the host never reads it outside fovpt_focus_state), the (r, tp) pairs of the last call (8 bytes per
    // pixel) and the context's own outputs; all allocated on first use
    struct FOVPT_LOCAL Focus { DevBuf state, rt; OutPair out; } focus;
    // fovpt_variance: two moment histories (M1, M2, n, z), used in turn by consecutive calls (last: the one the last call wrote), and
    // the context's own variance image; valid: a previous step exists, of size w x h (dropped by fovpt_variance_reset, fovpt_resize
    // and fovpt_set_scene); own_w x own_h: the frame size at which a step last wrote the context's own image (0: none since create /
    // resize).  fovpt_variance_filter: the level map, the ping-pong (I, v) buffers and the context's own outputs.  All allocated on
    // first use
    struct FOVPT_LOCAL Variance {
        DevBuf hist[2], image;
        int last = 0, w = 0, h = 0, own_w = 0, own_h = 0;
        bool valid = false;
        DevBuf level, j0, j1;
        OutPair out;
    } variance;
    // fovpt_quality: the context's own record(a fovpt_quality_sums, made by the first call that measures into it, which writes
    // every byte; the host reads it nowhere but in fovpt_quality_read) and the tile kernel's rows of partial sums
    // (fovpt_quality_rows of the frame's size); both allocated on first use
    struct FOVPT_LOCAL Quality { DevBuf sums, rows; } quality;
    // fovpt_packet_submit / fovpt_packet_wait (api_packet.hip), all made by a context's first submit: the copy stream, and per slot
    // the device buffer an encode writes (one each, so that an encode never overwrites a packet that is still being copied), the
    // pinned host buffer its copy fills (grown on demand), the event recorded on fovpt_stream() behind the encode, which the copy
    // stream waits for, and the event behind the copy, which fovpt_packet_wait and a later submit into the slot wait for.
    // pk_next: submits so far; submit k uses slot k % FOVPT_PACKET_SLOTS
    struct PacketSlot { DevBuf dev; void* host = nullptr; size_t host_bytes = 0, bytes = 0; hipEvent_t ev_encoded = nullptr, ev_done = nullptr; bool submitted = false; };
    PacketSlot pk_slot[FOVPT_PACKET_SLOTS];
    hipStream_t pk_stream = nullptr;
    unsigned pk_next = 0;
    // RCCL transport of the packed gather (fovpt_comm_init / fovpt_gather_frame)
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_world = 0;
    DevBuf comm_packed, comm_gathered;
    // stats
    fovpt_stats stats;
    // fovpt_warp_motion: what it asks of the last temporal step and of the last G-buffer trace, all on the host.  tm_step_blind
    // (set by every temporal step): the step ended an interval with an update the tracking did not see, so no mesh counts as
    // moved in it.  seq: one counter, incremented at each of the events below, whose value then is the event's stamp (0: never)
    // -- seq_frame: the last fovpt_render, fovpt_resize or fovpt_set_scene; seq_update: the last geometry update; seq_step: the
    // last temporal step; gb_stamp: the last G-buffer trace, 0 when it was not of the rendered frame's size and camera.  The hit
    // records (gbuffer.hit) describe the rendered frame and the current geometry when gb_stamp is above seq_frame and seq_update.
    bool tm_step_blind = false;
    uint64_t seq = 0, seq_frame = 0, seq_update = 0, seq_step = 0, gb_stamp = 0;
    uint64_t seq_adopt = 0;                // the last adoption of a background rebuild: no position moves, but the hit records of an earlier trace address the old hierarchy's triangle records
    ~fovpt_ctx();                          // what no DevBuf owns; fovpt_destroy synchronises first
};

int fail(fovpt_ctx* c, int code, const char* fmt, ...);       // sets the error text (c null: the text fovpt_last_error(NULL) returns), returns code
#define HIPCHK(c, x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail((c), FOVPT_E_DEVICE, "%s: %s", #x, hipGetErrorString(e_)); } while (0)
#define CHK(x) do { const int rc_ = (x); if (rc_) return rc_; } while (0)      // a step that has set the error text: its code goes up
int sync_all(fovpt_ctx* c);
SceneView scene_view(const fovpt_ctx* c);
void set_camera(FrameDev& fd, const fovpt_launch_params* lp);
void frame_levels(const fovpt_config& cfg, const fovpt_launch_params* lp, FrameDev& fd);
// fovpt_api.hip: the hierarchy build of fovpt_set_scene and the measurements of fovpt_hierarchy_cost, which a rebuild and a refit use
int build_hierarchy(fovpt_ctx* c, hipStream_t st, const float* d_flat, const uint32_t* d_mesh_of, uint32_t ntri, BvhBuildResult& br, float& ms);
int build_hierarchy(hipStream_t st, const BvhSwitches& sw, const float* d_flat, const uint32_t* d_mesh_of, uint32_t ntri, BvhBuildResult& br,
                    float& ms, char* err, size_t errlen);      // (no context: for a thread that is not the context's own)
void adopt_hierarchy(fovpt_ctx* c, const BvhBuildResult& br, float ms);
int enqueue_cost(fovpt_ctx* c, hipStream_t st, uint64_t update, fovpt_ctx::CostSlot** out);
int measure_built(fovpt_ctx* c);
// fovpt_api.hip: the pieces of the frame engine (run_passes / run_job) that the test hooks of api_debug.hip run a launch through.
// Hidden: the library does not export them.
#pragma GCC visibility push(hidden)
struct ProbePath { const uint32_t *guide_x, *guide_y; const float4* rec; int32_t row_mul; };
inline bool probe_complete(const fovpt_probe& p)              // what a launch needs of a probe: the texels, the four tables and a size
{
    return p.data && p.cdfValuesX && p.cdfValuesY && p.pdfValuesX && p.pdfValuesY && p.width > 0 && p.height > 0;
}
int ensure_state(fovpt_ctx* c, StateSet& S, size_t slots, size_t launches, hipStream_t st);   // S holds a job of that size (st: the stream about to use it)
PathState path_state(const fovpt_ctx* c, const StateSet& S);  // what the kernels see of a state set: its path state ...
RayQueue ray_queue(const StateSet& S, int k);                 // ... its k-th radiance-ray queue (0, 1) ...
ShadowQueue shadow_queue(const StateSet& S, int k);           // ... and its k-th shadow queue (0 .. FOVPT_NSQ - 1)
ProbePath probe_path(const fovpt_ctx* c, const fovpt_probe& probe);   // how a launch searches and reads the caller's probe
PassDev pass_from_lp(const fovpt_launch_params* lp, uint32_t gw, uint32_t gh);   // the pass of one fovpt_launch of a gw x gh grid
int frame_passes(const fovpt_config& cfg, fovpt_launch_params& L, PassDev* P);   // the passes of one fovpt_render; sets L's per-pass members
// the pass table of one job: `in` whole (row1 = 0: the rows 0 .. gh of each pass) or the launch rows [row0, row1) of each, as
// the passes first_pass, first_pass + 1, ... of the caller's frame (out may be in); *over: 0, or the job's sample slots when they
// exceed the budget of one job
int job_passes(fovpt_ctx* c, const PassDev* in, int npass, uint32_t first_pass, uint32_t row0, uint32_t row1, PassDev* out, uint64_t* over);
// what the kernels see of a job's frame, and its sample slots and launch records (accum_prev: what an accumulating resolve
// blends with when that is not the accum buffer itself -- the chunks of a pass --, else null)
int frame_dev(fovpt_ctx* c, const fovpt_launch_params* lp, const PassDev* passes_in, int npass, int chunked, int whole_frame,
              const fovpt_float4* accum_prev, FrameDev& fd, uint64_t& slots, uint64_t& launches);
#pragma GCC visibility pop
// api_animate.hip (fovpt_set_scene and the context's destructor drop what the update calls keep of a scene)
void drop_animation(fovpt_ctx* c);
// api_post.hip
int enqueue_gbuffer(fovpt_ctx* c, const fovpt_launch_params* lp, const FrameDev& view, GBufferDev& g, const char* who,
                    const GBufferDev* target = nullptr);
// api_post.hip: what fovpt_resize and fovpt_set_scene ask of the post-frame stages, and the steps the stages of api_post.hip and
// api_view.hip (and, for the first, api_packet.hip) share; `who` is the entry point's name, for the error text.  Hidden: the
// library does not export them.
#pragma GCC visibility push(hidden)
int post_resize(fovpt_ctx* c, int w, int h);         // what exists of the stages' buffers follows the frame; nothing is rendered at this size yet
int post_scene_changed(fovpt_ctx* c);                // (the device is idle) no history, the last trace is another scene's, exposure and focus start from scratch
int check_rendered_frame(fovpt_ctx* c, const fovpt_launch_params* lp, const char* who, const char* to_what, const char* need_guides, size_t limit);
int check_reserved(fovpt_ctx* c, const int32_t* words, int n, const char* who);
int check_aliases(fovpt_ctx* c, std::initializer_list<const void*> outs, std::initializer_list<const void*> ins, const char* who, const char* fmt_input);
// an edge-stopping scale of fovpt_denoise / fovpt_reconstruct: inside [FOVPT_SIGMA_MIN, FOVPT_SIGMA_MAX], so that 1 / sigma^2
// is a normal float and the denoiser's colour scale (1 / sigma^2) * 4^(FOVPT_DENOISE_MAX_ITERATIONS - 1) / 1e-4 stays finite
// (an infinite scale makes the centre tap 0 * inf: every weight 0, the output 0 / 0)
inline bool sigma_ok(float v) { return v >= FOVPT_SIGMA_MIN && v <= FOVPT_SIGMA_MAX; }
template <class T> bool zeroed(T* out) { if (out) memset(out, 0, sizeof(*out)); return out != nullptr; }      // how every fovpt_*_defaults begins
bool camera_inverse(const float* U, const float* V, const float* W, float* inv);
GBufferDev gbuffer_dev(const fovpt_ctx* c, const fovpt_gbuffer_ptrs* given);
int own_outputs(fovpt_ctx* c, const char* who, OutPair& own, fovpt_float4*& out_color, uint32_t*& out_rgba);
int own_buffers(fovpt_ctx* c, const char* who, OutPair& own, fovpt_float4** color, uint32_t** rgba);
int record_make(fovpt_ctx* c, DevBuf& rec, size_t bytes);
int record_reset(fovpt_ctx* c, DevBuf& rec, size_t bytes, hipStream_t st);
int record_read(fovpt_ctx* c, const DevBuf& rec, void* out, size_t bytes, const char* null_text);
#pragma GCC visibility pop
