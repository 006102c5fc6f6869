// fovpt_api.hip -- host side of libfovpt: the C ABI of include/fovpt.h over HIP.
//
// One context = one device = one stream, like the reference's SampleRenderer
// (PT_sv5_/SimplePathtracer.cpp:331-340).  Calls on a context are not thread-safe.
//
// Animated geometry is in api_animate.hip, the post-processing calls are in api_post.hip and api_view.hip, the multi-GPU gather in api_gather.hip, the
// frame packets in api_packet.hip, the test hooks (fovpt_debug_*) in api_debug.hip; fovpt_ctx.h is what they share.
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fovpt_ctx.h"

namespace {

std::string g_create_error;

}  // namespace

// for the context-free entry points of other translation units (model_loader.cpp): the text fovpt_last_error(NULL) returns
void fovpt_internal_set_error(const char* text) { g_create_error = text ? text : ""; }

int fail(fovpt_ctx* c, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

int sync_all(fovpt_ctx* c)
{
    for (int k = 0; k < c->engine.num_trace_streams; k++) HIPCHK(c, hipStreamSynchronize(c->engine.trace_stream[k]));
    if (c->shadow_stream) HIPCHK(c, hipStreamSynchronize(c->shadow_stream));      // last: the resolves wait for the lanes
    return FOVPT_OK;
}

// What the traversal and shading kernels see of the scene.
SceneView scene_view(const fovpt_ctx* c)
{
    SceneView sc;
    sc.nodes = c->nodes; sc.tris = c->tris; sc.tri_tc = (const float2*)c->tri_tc.p;
    sc.meshes = (const MeshDev*)c->meshes.p; sc.textures = (const TexDev*)c->textures.p;
    sc.num_tris = c->num_tris; sc.any_catcher = c->any_catcher;
    sc.tri_off = (uint32_t)((const char*)c->tris - (const char*)c->nodes);
    sc.num_nodes = c->stats.num_bvh_nodes;
    return sc;
}

// lp's camera into fd.eye / U / V / W
void set_camera(FrameDev& fd, const fovpt_launch_params* lp)
{
    const fovpt_float3* cam[4] = {&lp->camera.eye, &lp->camera.U, &lp->camera.V, &lp->camera.W};
    float* dst[4] = {fd.eye, fd.U, fd.V, fd.W};
    for (int k = 0; k < 4; k++) { dst[k][0] = cam[k]->x; dst[k][1] = cam[k]->y; dst[k][2] = cam[k]->z; }
}

namespace {

fovpt_config default_config()
{
    fovpt_config c;
    memset(&c, 0, sizeof(c));
    c.uniform = 0;
    c.r_inner = 74; c.r_outer = 241;                    // SimplePathtracer.cpp:20-21
    c.spp_periphery = 8; c.spp_middle = 16; c.spp_fovea = 32;   // :142,170,193
    c.spp_uniform = 4;                                  // :95
    c.max_depth = 4;                                    // deviceProgram.cu:515
    c.accumulate = 0;
    c.rank = 0; c.world = 1; c.tile_w = 8; c.tile_h = 4;
    return c;
}

// An integer knob of the environment: *dst = its value if the variable is set and lies in lo .. hi (atoi: text that is no number reads as 0)
bool env_int(const char* name, int lo, int hi, int* dst)
{
    const char* s = getenv(name);
    const int v = s ? atoi(s) : 0;
    if (!s || v < lo || v > hi) return false;
    *dst = v;
    return true;
}

hipEvent_t get_event(fovpt_ctx* c)
{
    if (!c->engine.free_events.empty()) { hipEvent_t e = c->engine.free_events.back(); c->engine.free_events.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;      // (Timed skips the measurement)
    return e;
}

struct Timed {
    fovpt_ctx* c; TimedKind kind; hipStream_t st; hipEvent_t a = nullptr, b = nullptr;
    Timed(fovpt_ctx* c_, TimedKind k, hipStream_t s = nullptr) : c(c_), kind(k), st(s ? s : c_->stream)
    {
        if (c->cfg.profile == 2) (void)sync_all(c);   // the kernel runs alone
        if (c->cfg.profile) {
            a = get_event(c); b = get_event(c);
            if (a && b) (void)hipEventRecord(a, st);
            else { if (a) c->engine.free_events.push_back(a); if (b) c->engine.free_events.push_back(b); a = b = nullptr; }
        }
    }
    ~Timed()
    {
        if (a && b) { (void)hipEventRecord(b, st); EventPair p = {a, b, kind}; c->engine.pending.push_back(p); }
        if (c->cfg.profile == 2) (void)hipStreamSynchronize(st);
    }
};

void drain_events(fovpt_ctx* c)
{
    for (auto& p : c->engine.pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            switch (p.kind) {
            case T_GENERATE: c->stats.ms_generate += ms; break;
            case T_TRACE: c->stats.ms_trace += ms; c->stats.n_trace_launches++; break;
            case T_SHADE: c->stats.ms_shade += ms; break;
            case T_SHADOW: c->stats.ms_shadow += ms; c->stats.n_shadow_launches++; break;
            case T_RESOLVE: c->stats.ms_resolve += ms; break;
            }
        }
        c->engine.free_events.push_back(p.a); c->engine.free_events.push_back(p.b);
    }
    c->engine.pending.clear();
}

void free_scene(fovpt_ctx* c)
{
    if (c->nodes) (void)hipFree(c->nodes);          // (the triangles live in the same allocation, behind the nodes)
    c->nodes = nullptr; c->tris = nullptr;
    for (void* p : c->tex_pixels) (void)hipFree(p);
    c->tex_pixels.clear();
    c->has_scene = false;
    drop_animation(c);                              // what the update calls keep of it (api_animate.hip)
}

// The engine of a new context (c->num_cus is set): the launch grids, the knobs of the environment switches (tuning and A/B only;
// none changes a result), the streams of every lane and the events of every state set.  Returns the first HIP error; what was
// made until then is the destructor's.
hipError_t make_engine(fovpt_ctx* c)
{
    Engine& E = c->engine;
    // Blocks per CU, each a default that the switch of that name replaces when it lies in range; every grid a multiple of
    // FOVPT_SHARDS (shard_grid).
    //   generate: 8 blocks of 256 = 32 waves per CU, grid-stride
    //   closest-hit launches, in units of 256 threads (k_traverse's own blocks are FOVPT_TBLOCK threads)
    //   occlusion launches (measured best of 2..8 with per-wave ray pools)
    //   shading: the kernel holds 4 waves per SIMD (104 VGPRs) = 4 blocks per CU; twice the resident number of blocks is
    //   measured best (blocks per CU 2 / 3 / 4 / 6 / 8: shading 0.307 / 0.274 / 0.261 / 0.263 / 0.244 ms per C3 frame)
    const struct { const char* name; int hi, per_cu; int* grid; } grids[4] = {
        {"FOVPT_GRID_GEN", 64, 8, &E.grid}, {"FOVPT_GRID", 64, FOVPT_GRID_PER_CU, &E.grid_trace},
        {"FOVPT_GRID_SHADOW", 16, FOVPT_GRID_SHADOW_PER_CU, &E.grid_shadow}, {"FOVPT_GRID_SHADE", 16, 8, &E.grid_shade}};
    for (const auto& g : grids) {
        int per_cu = g.per_cu;
        (void)env_int(g.name, 1, g.hi, &per_cu);
        *g.grid = shard_grid(c->num_cus * per_cu);
    }
    if (const char* sb = getenv("FOVPT_SLOT_BUDGET")) { const long long v = atoll(sb); if (v > 0) E.slot_budget = (uint64_t)v; }   // tests: force chunking
    (void)env_int("FOVPT_LANES", 1, FOVPT_MAX_LANES, &E.knobs.lanes);
    (void)env_int("FOVPT_SPREAD_OCCLUSION", INT_MIN, INT_MAX, &E.knobs.spread_occlusion);      // 0 off, 1 the last occlusion launch, 2 the second (A/B); not range-checked
    (void)env_int("FOVPT_CHAINS", 1, 2, &E.knobs.chains_default);
    int nsets = 2 * E.knobs.lanes;
    (void)env_int("FOVPT_SETS", 2, 2 * FOVPT_MAX_LANES, &nsets);
    E.knobs.nsets = (unsigned)nsets;
    // the main chain is the critical path: give it the higher priority so occlusion waves only fill gaps
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    hipError_t e = hipStreamCreateWithPriority(&c->stream, hipStreamDefault, prio_hi);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&c->shadow_stream, hipStreamDefault, prio_lo);
    E.lane_main[0] = c->stream; E.lane_shadow[0] = c->shadow_stream;
    for (int l = 1; l < E.knobs.lanes; l++) {
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&E.lane_main[l], hipStreamDefault, prio_hi);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&E.lane_shadow[l], hipStreamDefault, prio_lo);
    }
    for (int l = 0; l < FOVPT_MAX_LANES; l++)
        for (hipStream_t s : {E.lane_main[l], E.lane_shadow[l]})
            if (s && s != c->shadow_stream) E.trace_stream[E.num_trace_streams++] = s;
    for (StateSet& S : E.set) {
        for (ChainEvents& ch : S.chain)
            for (int k = 0; k <= FOVPT_MAX_ITERS && e == hipSuccess; k++) {
                e = hipEventCreateWithFlags(&ch.shade[k], hipEventDefault);
                if (e == hipSuccess) e = hipEventCreateWithFlags(&ch.shadow[k], hipEventDefault);
            }
        if (e == hipSuccess) e = hipEventCreateWithFlags(&S.ev_done, hipEventDefault);
    }
    return e;
}

}  // namespace

int ensure_state(fovpt_ctx* c, StateSet& S, size_t slots, size_t launches, hipStream_t st)
{
    const size_t v = 16;
    HIPCHK(c, S.s_thr.reserve(slots * v)); HIPCHK(c, S.s_rng.reserve(slots * v));
    HIPCHK(c, S.s_hit.reserve((size_t)shard_capacity(slots) * FOVPT_SHARDS * v));      // indexed like the ray queues
    HIPCHK(c, S.s_alpha.reserve(slots * v));
    HIPCHK(c, S.s_rad.reserve(slots * v * (size_t)c->cfg.max_depth));
    HIPCHK(c, S.s_backplate.reserve(launches * v));
    if (c->cfg.write_guides) { HIPCHK(c, S.s_guide_n.reserve(slots * v)); HIPCHK(c, S.s_guide_a.reserve(slots * v)); }
    // sharded queues: FOVPT_SHARDS regions of shard_capacity(slots) entries each;
    // there is one shadow queue per bounce in flight (FOVPT_NSQ): bounce it's occlusion rays may still be running
    // on the shadow stream while later bounces are shaded
    const size_t qn = (size_t)shard_capacity(slots) * FOVPT_SHARDS;
    for (int k = 0; k < 2; k++) { HIPCHK(c, S.q_o[k].reserve(qn * v)); HIPCHK(c, S.q_d[k].reserve(qn * v)); }
    const int iters_max = c->cfg.max_depth + (c->any_catcher ? 25 : 0);
    for (int k = 0; k < FOVPT_NSQ && k < iters_max; k++) {
        HIPCHK(c, S.sq_o[k].reserve(qn * v)); HIPCHK(c, S.sq_d[k].reserve(qn * v));
        HIPCHK(c, S.sq_vis[k].reserve(qn * v)); HIPCHK(c, S.sq_occ[k].reserve(qn * v));
    }
    if (!S.counters.p) {
        HIPCHK(c, S.counters.reserve(sizeof(Counters)));
        HIPCHK(c, hipMemsetAsync(S.counters.p, 0, sizeof(Counters), st));      // (the main stream of the job that is about to use the set)
        HIPCHK(c, hipStreamSynchronize(st));                                   // once per set: a second chain starts on another stream
    }
    return FOVPT_OK;
}

// The other sets of a rotation through nrot sets, grown to the job's size now rather than one per job: an allocation waits for
// the device, and the first jobs of a caller that keeps several frames in flight would each stop for one.  Only a set too small
// for the job's sample slots: ensure_state would also give a set that is large enough a longer backplate, guide buffers the
// configuration has since switched on, or more shadow queues (a scene that has gained a catcher) -- allocations, and a wait
// each, that this job does not need; the set gets them when its own job comes.
int grow_rotation(fovpt_ctx* c, unsigned nrot, unsigned set_index, size_t slots, size_t launches, hipStream_t st)
{
    for (unsigned k = 0; k < nrot; k++) {
        const StateSet& S = c->engine.set[k];
        if (k != set_index && (S.s_thr.bytes < slots * 16 || S.s_rad.bytes < slots * 16 * (size_t)c->cfg.max_depth))
            CHK(ensure_state(c, c->engine.set[k], slots, launches, st));
    }
    return FOVPT_OK;
}

// What the kernels see of a state set: its path state (the guide pointers null unless write_guides is on: ensure_state's rule) ...
PathState path_state(const fovpt_ctx* c, const StateSet& S)
{
    PathState ps;
    memset(&ps, 0, sizeof(ps));
    ps.thr = (float4*)S.s_thr.p; ps.rng = (uint4*)S.s_rng.p; ps.hit = (float4*)S.s_hit.p; ps.rad = (float4*)S.s_rad.p;
    ps.stride = (size_t)c->cfg.max_depth; ps.alpha = (float4*)S.s_alpha.p; ps.backplate = (float4*)S.s_backplate.p;
    if (c->cfg.write_guides) { ps.guide_n = (float4*)S.s_guide_n.p; ps.guide_a = (float4*)S.s_guide_a.p; }
    return ps;
}

// ... its k-th radiance-ray queue ...
RayQueue ray_queue(const StateSet& S, int k) { return RayQueue{(float4*)S.q_o[k].p, (float4*)S.q_d[k].p}; }

// ... and its k-th shadow queue
ShadowQueue shadow_queue(const StateSet& S, int k)
{
    ShadowQueue sq;
    sq.o = (float4*)S.sq_o[k].p; sq.d = (float4*)S.sq_d[k].p; sq.val_vis = (float4*)S.sq_vis[k].p; sq.val_occ = (float4*)S.sq_occ[k].p;
    return sq;
}

static int run_job(fovpt_ctx* c, const fovpt_launch_params* lp, const PassDev* passes, int npass, int chunked, int whole_frame, const fovpt_float4* accum_prev);

// The pass table of one job (pass_table, fovpt_jobplan.h), for run_passes (a whole frame, a chunk) and for the hooks of
// api_debug.hip, so that a test runs the frame a job would: every pass of `in` whole (row1 = 0) or its launch rows [row0, row1), as
// the passes first_pass, first_pass + 1, ... of the caller's frame -- ownership rotates with a pass's place in the frame, also when
// it runs as a job of its own.  *over: 0, or the job's sample slots when they exceed the budget of one job.
int job_passes(fovpt_ctx* c, const PassDev* in, int npass, uint32_t first_pass, uint32_t row0, uint32_t row1, PassDev* out, uint64_t* over)
{
    uint64_t slots = 0;
    if (!pass_table(in, npass, first_pass, row0, row1, out, &slots))
        return fail(c, FOVPT_E_INVALID, "samples_per_launch must be >= 1 (do{}while(--i), deviceProgram.cu:448,539)");
    *over = slots > c->engine.slot_budget ? slots : 0;      // (a job without sample slots fits)
    return FOVPT_OK;
}

// The engine: all passes of one frame as one wavefront job (or several, for very large launches).
// whole_frame: the passes are a complete frame (fovpt_render), so with world > 1 the pixels nobody writes are
// cleared on the ranks other than 0 (rank 0 keeps them, as the reference's frame buffer keeps what no launch
// overwrites): the sum over the ranks is then the single-GPU frame.  A single fovpt_launch leaves them alone on
// every rank -- it may be one of several launches that make up the caller's frame.
static int run_passes(fovpt_ctx* c, const fovpt_launch_params* lp, const PassDev* passes_in, int npass, int whole_frame)
{
    if (!c->has_scene || lp->traversable != c->scene_id) return fail(c, FOVPT_E_NO_SCENE, "launch without a scene (traversable %llu, current %llu)",
                                                                     (unsigned long long)lp->traversable, (unsigned long long)c->scene_id);
    if (!probe_complete(lp->probe)) return fail(c, FOVPT_E_NO_PROBE, "launch with an incomplete probe");
    if (!lp->frame.accum_buffer || !lp->frame.frame_buffer) return fail(c, FOVPT_E_NO_FRAME, "launch with null frame buffers");
    if (lp->frame.size.x <= 0 || lp->frame.size.y <= 0) return fail(c, FOVPT_E_INVALID, "bad frame size");
    if (c->cfg.max_depth < 1 || c->cfg.max_depth > 32) return fail(c, FOVPT_E_INVALID, "max_depth out of range");

    PassDev job[FOVPT_MAX_PASSES];
    uint64_t over = 0;
    CHK(job_passes(c, passes_in, npass, 0u, 0u, 0u, job, &over));
    c->stats.frames++;
    if (!over) return run_job(c, lp, job, npass, 0, whole_frame, nullptr);

    // A launch whose sample slots would not fit the per-job budget is cut into chunks of launch rows and
    // run as several jobs in the reference's order (pass by pass, rows ascending): later jobs overwrite
    // earlier ones exactly as later launch indices overwrite earlier ones in the reference.
    const uint64_t budget = c->engine.slot_budget;
    const size_t npix = (size_t)lp->frame.size.x * lp->frame.size.y;
    for (int p = 0; p < npass; p++) {
        const PassDev& P = passes_in[p];
        // Accumulate mode blends with the pixel's value from BEFORE the launch (a pass of render() = one optixLaunch).  The
        // chunks of a pass are separate jobs, so a pixel that two of them write (clamped or overlapping fills) would otherwise
        // be blended twice: a pass that blends gets a copy, taken before its first chunk, for its chunks to read.  For the first
        // pass that is before anything of this frame touches the buffer, the clearing below included.  (render() blends in pass
        // P only, which is the first: no caller of this library takes the copy for a later pass.)
        const bool blends = c->cfg.accumulate && P.subframe > 0 && !P.redraw;
        if (blends) {
            HIPCHK(c, c->engine.accum_before.reserve(npix * 16));
            HIPCHK(c, hipMemcpyAsync(c->engine.accum_before.p, lp->frame.accum_buffer, npix * 16, hipMemcpyDeviceToDevice, c->shadow_stream));
        }
        if (p == 0 && whole_frame && c->cfg.world > 1 && c->cfg.rank != 0) {
            // The chunk jobs zero the pixels whose last writer (within the chunk) belongs to another rank; pixels no
            // chunk writes must not keep this rank's stale values (rank 0 keeps its own, like the unchunked path)
            // (on the stream the resolves run on: after the previous frame's, before this frame's)
            HIPCHK(c, hipMemsetAsync(lp->frame.frame_buffer, 0, npix * 4, c->shadow_stream));
            HIPCHK(c, hipMemsetAsync(lp->frame.accum_buffer, 0, npix * 16, c->shadow_stream));
        }
        if (P.gw == 0 || P.gh == 0) continue;
        const ChunkRows cr = chunk_rows(budget, P.gw, P.spp);
        if (cr.rows == 0) return fail(c, FOVPT_E_INVALID, "one launch row needs %llu sample slots (budget %llu)", (unsigned long long)cr.per_row, (unsigned long long)budget);
        for (uint32_t y0 = 0; y0 < P.gh; y0 += cr.rows) {
            PassDev Q;                         // the job holds ONE pass
            CHK(job_passes(c, &P, 1, (uint32_t)p, y0, y0 + cr.rows < P.gh ? y0 + cr.rows : P.gh, &Q, &over));
            CHK(run_job(c, lp, &Q, 1, 1, 0, blends ? (const fovpt_float4*)c->engine.accum_before.p : nullptr));
        }
    }
    return FOVPT_OK;
}

// How a launch searches and reads the caller's probe: the guide tables, the packed records and the one-row layout belong to the
// probe this context uploaded.  One function for run_job and for the debug entry points, so that a test sees the path a frame takes.
ProbePath probe_path(const fovpt_ctx* c, const fovpt_probe& probe)
{
    ProbePath pp;
    // the guide tables belong to the probe this context uploaded; a caller-supplied foreign probe is searched plainly
    const bool own_probe = c->guide_ok && probe.cdfValuesX == (float*)c->pr_cdfx.p && probe.cdfValuesY == (float*)c->pr_cdfy.p
                           && probe.width == c->guide_w && probe.height == c->guide_h;
    pp.guide_x = own_probe ? (const uint32_t*)c->pr_guidex.p : nullptr;
    pp.guide_y = own_probe ? (const uint32_t*)c->pr_guidey.p : nullptr;
    // (a probe whose rows are all alike is served from ONE row of the split arrays, which stays in L1; its 32-byte records would not)
    pp.rec = (own_probe && !c->rows_identical && probe.data == (fovpt_float4*)c->pr_data.p && probe.pdfValuesX == (float*)c->pr_pdfx.p)
             ? (const float4*)c->pr_rec.p : nullptr;
    pp.row_mul = (c->rows_identical && probe.data == (fovpt_float4*)c->pr_data.p && probe.pdfValuesX == (float*)c->pr_pdfx.p
                  && probe.cdfValuesX == (float*)c->pr_cdfx.p && probe.width == c->guide_w && probe.height == c->guide_h) ? 0 : 1;
    return pp;
}

// What the kernels see of a frame: the passes (with their places in the job's sample slots and launch records), the camera, the
// probe and how it is searched, the caller's frame buffers and the configuration.  One function for run_job and for
// the resolve and generate hooks of api_debug.hip, so that a test hook runs the frame a job of the same parameters would.
// accum_prev: what an accumulating resolve blends with when that is not the accum buffer itself (the chunks of a pass: run_passes).
int frame_dev(fovpt_ctx* c, const fovpt_launch_params* lp, const PassDev* passes_in, int npass, int chunked, int whole_frame,
              const fovpt_float4* accum_prev, FrameDev& fd, uint64_t& slots, uint64_t& launches)
{
    memset(&fd, 0, sizeof(fd));
    fd.chunked = chunked;
    fd.zero_holes = (whole_frame && !chunked && c->cfg.world > 1 && c->cfg.rank != 0) ? 1 : 0;
    slots = 0; launches = 0;
    for (int p = 0; p < npass; p++) {
        PassDev P = passes_in[p];
        const uint64_t rows = P.row1 - P.row0;
        P.slot_base = (uint32_t)slots; P.launch_base = (uint32_t)launches;
        slots += (uint64_t)P.gw * rows * P.spp;
        launches += (uint64_t)P.gw * rows;
        fd.pass[p] = P;
    }
    if (slots >= (1ull << 31)) return fail(c, FOVPT_E_INVALID, "launch too large: %llu sample slots", (unsigned long long)slots);
    fd.npass = npass;
    fd.w = lp->frame.size.x; fd.h = lp->frame.size.y;
    fd.cx = lp->frame.c.x; fd.cy = lp->frame.c.y;
    set_camera(fd, lp);
    fd.probe = lp->probe;
    const ProbePath pp = probe_path(c, lp->probe);
    fd.guide_x = pp.guide_x; fd.guide_y = pp.guide_y; fd.probe_rec = pp.rec; fd.probe_row_mul = pp.row_mul;
    fd.accum = lp->frame.accum_buffer;
    fd.accum_prev = accum_prev ? accum_prev : lp->frame.accum_buffer;
    fd.frame = lp->frame.frame_buffer;
    if (c->cfg.write_guides) {
        if (c->any_catcher) return fail(c, FOVPT_E_INVALID, "write_guides is not available with shadow-catcher materials");
        fd.g_normal = lp->frame.normal_buffer; fd.g_color = lp->frame.color_buffer; fd.g_albedo = lp->frame.albedo_buffer;
    }
    fd.total_slots = (uint32_t)slots;
    fd.max_depth = c->cfg.max_depth;
    fd.accumulate = c->cfg.accumulate;
    fd.options = c->cfg.options;
    fd.partition = !c->cfg.uniform;      // direction classes in k_shade's appends: foveated frames gain, uniform ones lose
    fd.rank = c->cfg.rank; fd.world = c->cfg.world < 1 ? 1 : c->cfg.world;
    fd.tile_w = c->cfg.tile_w > 0 ? c->cfg.tile_w : 8; fd.tile_h = c->cfg.tile_h > 0 ? c->cfg.tile_h : 4;
    return FOVPT_OK;
}

// What every chain of a job shares: the frame, the set's path state, queues and counters, the scene, and the plan's iterations
struct JobShared {
    FrameDev fd;
    PathState ps;
    SceneView sc;
    RayQueue q[2];
    ShadowQueue sq[FOVPT_NSQ];
    Counters* cnt;
    uint32_t cap;
    int iters, nsq, spread_it;
};

// One chain of a job (ChainPlan, fovpt_jobplan.h) on its lane's streams, its launches' completion events in ev:
// Main chain (stream `st`):    generate, closest(0), shade(0), closest(1), shade(1), ... shade(D-1)
// Shadow chain (stream `ss`):  occlusion(it) as soon as shade(it) has queued its rays; then resolve.
// Every radiance cell has one writer, so the only joins are: shade(it+2) reuses the shadow queue
// buffer of bounce it, and resolve needs everything -- it runs on the shadow stream, behind the last
// occlusion launch (which waited for the last shade), so the main chain is free for the next job.
static int issue_chain(fovpt_ctx* c, const JobShared& J, const ChainPlan& ch, const ChainEvents& ev)
{
    const Engine& E = c->engine;
    const hipStream_t st = E.lane_main[ch.lane], ss = E.lane_shadow[ch.lane];
    const uint32_t sel = ch.sel, cap = J.cap;
    const int iters = J.iters, nsq = J.nsq;
    RayQueue qa = J.q[0], qb = J.q[1];
    const int g_gen = E.grid / ch.div, g_trace = E.grid_trace / ch.div, g_shadow = E.grid_shadow / ch.div, g_shade = E.grid_shade / ch.div;
    { Timed t(c, T_GENERATE, st); (void)fovpt_launch_generate(st, J.fd, J.ps, qa, cap, J.cnt, ch.slot_begin, ch.slot_end, g_gen, sel); }
    { Timed t(c, T_TRACE, st); fovpt_launch_traverse(st, J.sc, J.ps, qa, J.sq[0], cap, J.cnt, 0, -1, g_trace, nullptr, sel); }
    for (int it = 0; it < iters; it++) {
        if (it >= nsq) HIPCHK(c, hipStreamWaitEvent(st, ev.shadow[it - nsq], 0));
        // the events ride on the kernels' own completion signals (hipExtLaunchKernel): a separate
        // hipEventRecord would put a marker packet between shade(it) and closest(it+1), ~6 us on the critical path
        { Timed t(c, T_SHADE, st); fovpt_launch_shade(st, J.fd, J.sc, J.ps, qa, qb, J.sq[it % nsq], cap, J.cnt, it, g_shade, ev.shade[it], sel); }
        // (a sharded frame on the first lane: bounce spread_it's occlusion rays run on the OTHER lane's shadow stream -- the
        // completion stream carries every job's resolve as well; the resolve waits for it)
        const hipStream_t so = it == J.spread_it ? E.lane_shadow[1] : ss;
        HIPCHK(c, hipStreamWaitEvent(ss, ev.shade[it], 0));
        if (so != ss) HIPCHK(c, hipStreamWaitEvent(so, ev.shade[it], 0));
        { Timed t(c, T_SHADOW, so); fovpt_launch_traverse(so, J.sc, J.ps, qb, J.sq[it % nsq], cap, J.cnt, -1, it, g_shadow, ev.shadow[it], sel); }
        if (it + 1 < iters) { Timed t(c, T_TRACE, st); fovpt_launch_traverse(st, J.sc, J.ps, qb, J.sq[0], cap, J.cnt, it + 1, -1, g_trace, nullptr, sel); }
        const RayQueue tmp = qa; qa = qb; qb = tmp;
    }
    return FOVPT_OK;
}

// One wavefront job: generate -> (closest, shade, occlusion) x depth -> resolve over the given passes / row ranges.
static int run_job(fovpt_ctx* c, const fovpt_launch_params* lp, const PassDev* passes, int npass, int chunked, int whole_frame, const fovpt_float4* accum_prev)
{
    Engine& E = c->engine;
    JobShared J;
    uint64_t slots = 0, launches = 0;
    CHK(frame_dev(c, lp, passes, npass, chunked, whole_frame, accum_prev, J.fd, slots, launches));
    if (slots == 0) return FOVPT_OK;
    const PlanJob job = {c->cfg.frames_in_flight, c->cfg.chains_per_frame, c->cfg.max_depth, c->cfg.world, c->any_catcher, slots, chunked};
    const JobPlan plan = plan_job(E.knobs, E.rot, job);

    // wait for the scene.  A refit enqueued on fovpt_stream() since the last job (fovpt_update_vertices): every stream that may
    // trace the scene or read its triangle records -- the lanes' main and shadow streams, both chains' -- waits for it, once
    // (what runs on shadow_stream itself is behind it already)
    if (E.refit_pending) {
        for (int k = 0; k < E.num_trace_streams; k++) HIPCHK(c, hipStreamWaitEvent(E.trace_stream[k], c->ev_scene, 0));
        E.refit_pending = false;
    }

    // take the set.  It is free once the resolve of the job that used it last has run (reserve() may also free and
    // reallocate its buffers, which the runtime orders after all device work); its counters are made and cleared on the
    // stream about to use it
    StateSet& S = E.set[plan.set_index];
    const hipStream_t st = E.lane_main[plan.chain[0].lane];
    for (int k = 0; k < plan.nchains && S.used; k++) HIPCHK(c, hipStreamWaitEvent(E.lane_main[plan.chain[k].lane], S.ev_done, 0));
    CHK(ensure_state(c, S, (size_t)slots, (size_t)launches, st));
    if (!chunked) CHK(grow_rotation(c, plan.nrot, plan.set_index, (size_t)slots, (size_t)launches, st));
    E.rot.jobs++;
    E.rot.last_set = plan.set_index;
    S.used = true;

    J.ps = path_state(c, S);
    J.sc = scene_view(c);
    for (int k = 0; k < 2; k++) J.q[k] = ray_queue(S, k);
    for (int k = 0; k < FOVPT_NSQ; k++) J.sq[k] = shadow_queue(S, k);
    J.cnt = (Counters*)S.counters.p;
    // (the queue counters are zero: at allocation, and again by the resolve of the set's previous job)
#if FOVPT_V_STEPSTAT
    HIPCHK(c, hipMemsetAsync(J.cnt, 0, offsetof(Counters, stat_radiance), st));      // the diagnostic build keeps them after the job
#endif
    J.cap = shard_capacity(slots);
    J.iters = plan.iters; J.nsq = plan.nsq; J.spread_it = plan.spread_it;
    for (int k = 0; k < plan.nchains; k++) CHK(issue_chain(c, J, plan.chain[k], S.chain[k]));

    // join and resolve.  Every resolve runs on shadow_stream, whatever the lane: in job order (a later job's pixels overwrite, or
    // blend with, an earlier one's), behind whatever the caller has queued on fovpt_stream() since the previous frame, and in front
    // of what it queues next.  A chain of another lane joins it behind its last occlusion launch (which waited for its last
    // shade; the first lane's last occlusion launch IS on shadow_stream), and so does the occlusion launch that was moved there.
    for (int k = 0; k < plan.nchains; k++)
        if (E.lane_shadow[plan.chain[k].lane] != c->shadow_stream) HIPCHK(c, hipStreamWaitEvent(c->shadow_stream, S.chain[k].shadow[plan.iters - 1], 0));
    if (plan.spread_it >= 0) HIPCHK(c, hipStreamWaitEvent(c->shadow_stream, S.chain[0].shadow[plan.spread_it], 0));
    { Timed t(c, T_RESOLVE, c->shadow_stream); fovpt_launch_resolve(c->shadow_stream, J.fd, J.ps, J.cnt, S.ev_done); }
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

PassDev pass_from_lp(const fovpt_launch_params* lp, uint32_t gw, uint32_t gh)
{
    PassDev P;
    memset(&P, 0, sizeof(P));
    P.gw = gw; P.gh = gh;
    P.fx = lp->frame.factor.x; P.fy = lp->frame.factor.y; P.fz = lp->frame.factor.z;
    P.fill = lp->frame.fillSize;
    P.offx = lp->frame.offset.x; P.offy = lp->frame.offset.y;
    P.r_inner = lp->frame.r_inner; P.r_outer = lp->frame.r_outer;
    P.spp = lp->samples_per_launch;
    P.subframe = lp->frame.subframe_index;
    P.redraw = lp->frame.redraw;
    return P;
}

// The launches of one SampleRenderer::render() call (SimplePathtracer.cpp:77-214): sets the per-pass members of L the
// way the reference leaves them after its last launch and returns the passes.  (The caller restores subframe_index.)
int frame_passes(const fovpt_config& cfg, fovpt_launch_params& L, PassDev* P)
{
    if (cfg.uniform) {                                                                       // FOV_OFF :85-131
        L.frame.subframe_index = 0;
        L.frame.factor.x = L.frame.factor.y = L.frame.factor.z = 1;
        L.frame.fillSize = 1;
        L.frame.r_outer = 1000000000;
        L.frame.r_inner = 0;
        L.samples_per_launch = (uint32_t)cfg.spp_uniform;
        L.frame.offset.x = L.frame.offset.y = 0;
        L.frame.redraw = 0;
        L.viewportSize.x = L.frame.size.x; L.viewportSize.y = L.frame.size.y;
        P[0] = pass_from_lp(&L, (uint32_t)L.frame.size.x, (uint32_t)L.frame.size.y);
        return 1;
    }
    const int inner_radius = cfg.r_inner, outer_radius = cfg.r_outer;
    // periphery :137-157
    L.frame.factor.x = 4; L.frame.factor.y = 4; L.frame.factor.z = 1;
    L.frame.fillSize = 4;
    L.frame.r_outer = 1000000000;
    L.frame.r_inner = (float)outer_radius;
    L.samples_per_launch = (uint32_t)cfg.spp_periphery;
    L.frame.offset.x = L.frame.offset.y = 0;
    L.frame.redraw = 0;
    P[0] = pass_from_lp(&L, (uint32_t)(L.frame.size.x / 4), (uint32_t)(L.frame.size.y / 4));
    // intermediate :160-187
    L.frame.subframe_index = 0;
    L.frame.factor.x = 2; L.frame.factor.y = 2; L.frame.factor.z = 1;
    L.frame.fillSize = 2;
    L.frame.r_outer = (float)(outer_radius + 2);
    L.frame.r_inner = (float)inner_radius;
    L.samples_per_launch = (uint32_t)cfg.spp_middle;
    L.frame.offset.x = L.frame.c.x - (uint32_t)(outer_radius + 2);
    L.frame.offset.y = L.frame.c.y - (uint32_t)(outer_radius + 2);
    L.frame.redraw = 1;
    P[1] = pass_from_lp(&L, (uint32_t)L.frame.r_outer, (uint32_t)L.frame.r_outer);
    // fovea :189-209
    L.frame.factor.x = 1; L.frame.factor.y = 1; L.frame.factor.z = 1;
    L.frame.fillSize = 1;
    L.frame.r_outer = (float)(inner_radius + 1);
    L.frame.r_inner = 0;
    L.samples_per_launch = (uint32_t)cfg.spp_fovea;
    L.frame.offset.x = L.frame.c.x - (uint32_t)(inner_radius + 1);
    L.frame.offset.y = L.frame.c.y - (uint32_t)(inner_radius + 1);
    L.frame.redraw = 1;
    P[2] = pass_from_lp(&L, (uint32_t)(L.frame.r_outer * 2), (uint32_t)(L.frame.r_outer * 2));
    return 3;
}

// The hierarchy over d_flat (9 floats per triangle) on stream st, as fovpt_set_scene builds it: sw (FOVPT_BVH, FOVPT_SPLIT, ...,
// read by the caller), and a second build without reinsertion when reinsertion made the tree too deep; *ms = its device time.
// On success br holds the new hierarchy (adopt_hierarchy takes it); on failure nothing is kept, the code is returned and err
// holds the text.  Touches no context: whoever sees the result on the context's own thread calls fail() with it (a background
// rebuild runs this on a thread of its own).
int build_hierarchy(hipStream_t st, const BvhSwitches& sw, const float* d_flat, const uint32_t* d_mesh_of, uint32_t ntri, BvhBuildResult& br,
                    float& ms, char* err, size_t errlen)
{
#define BHCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { snprintf(err, errlen, "%s: %s", #x, hipGetErrorString(e_)); return FOVPT_E_DEVICE; } } while (0)
    struct Ev { hipEvent_t e = nullptr; ~Ev() { if (e) (void)hipEventDestroy(e); } } ev0, ev1;    // destroyed on every return path
    err[0] = 0;
    BHCHK(hipEventCreate(&ev0.e)); BHCHK(hipEventCreate(&ev1.e));
    const hipEvent_t e0 = ev0.e, e1 = ev1.e;
    BHCHK(hipEventRecord(e0, st));
#undef BHCHK
    memset(&br, 0, sizeof(br));
    char errbuf[256];
    hipError_t be = fovpt_build_lbvh(st, d_flat, d_mesh_of, ntri, sw, -1, &br, errbuf, sizeof(errbuf));
    if (be == hipSuccess && br.reinserted && 3 * br.max_depth + 1 > FOVPT_STACK) {
        // reinsertion lowers the tree's cost, not its depth: a hierarchy it made too deep for the traversal stack is built again without it
        free_hierarchy(br);
        be = fovpt_build_lbvh(st, d_flat, d_mesh_of, ntri, sw, 0, &br, errbuf, sizeof(errbuf));
    }
    (void)hipEventRecord(e1, st);
    (void)hipEventSynchronize(e1);
    ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    if (be != hipSuccess) { snprintf(err, errlen, "LBVH build: %s", errbuf); return FOVPT_E_DEVICE; }
    if (3 * br.max_depth + 1 > FOVPT_STACK) {       // a wide node leaves at most 3 entries behind
        snprintf(err, errlen, "hierarchy depth %u needs more than the %d traversal stack entries", br.max_depth, FOVPT_STACK);
        free_hierarchy(br);
        return FOVPT_E_BVH_DEPTH;
    }
    if ((size_t)((const char*)br.tris - (const char*)br.nodes) + br.tri_bytes + 64 >= (1ull << 32)) {
        snprintf(err, errlen, "hierarchy of %llu bytes exceeds the 32-bit offsets of the traversal", (unsigned long long)(br.node_bytes + br.tri_bytes));
        free_hierarchy(br);
        return FOVPT_E_INVALID;
    }
    return FOVPT_OK;
}

// build_hierarchy for a caller on the context's own thread: the switches are the environment's now, the text goes to the context
int build_hierarchy(fovpt_ctx* c, hipStream_t st, const float* d_flat, const uint32_t* d_mesh_of, uint32_t ntri, BvhBuildResult& br, float& ms)
{
    char err[384];
    const int rc = build_hierarchy(st, fovpt_bvh_switches(), d_flat, d_mesh_of, ntri, br, ms, err, sizeof(err));
    return rc ? fail(c, rc, "%s", err) : FOVPT_OK;
}

namespace {

// The device arrays of a width x height probe (the device is idle): the texels and the four tables
int reserve_probe(fovpt_ctx* c, int width, int height)
{
    const size_t n = (size_t)width * height;
    HIPCHK(c, c->pr_pdfx.reserve(n * 4)); HIPCHK(c, c->pr_cdfx.reserve(n * 4));
    HIPCHK(c, c->pr_pdfy.reserve((size_t)height * 4)); HIPCHK(c, c->pr_cdfy.reserve((size_t)height * 4));
    HIPCHK(c, c->pr_data.reserve(n * 16));
    return FOVPT_OK;
}

// What fovpt_set_probe and fovpt_set_probe_data share once the probe's arrays are on the device: whether the CDFs (host copies
// cdfX, cdfY) are sorted, the guide tables and packed records if so, whether all rows are alike (texels, cdfX, and pdfX where
// the caller has it on the host), and the caller's fovpt_probe.
int finish_probe(fovpt_ctx* c, int width, int height, const fovpt_float4* data, const float* pdfX, const float* cdfX, const float* cdfY,
                 const fovpt_float3* offset, fovpt_probe* out)
{
    const size_t n = (size_t)width * height;
    // guide tables for the two CDF searches of ProbeSample: only valid on non-decreasing CDFs
    bool sorted = true;
    for (int row = 0; row < height && sorted; row++) {
        const float* cr = cdfX + (size_t)row * width;
        for (int k = 1; k < width; k++) if (!(cr[k] >= cr[k - 1])) { sorted = false; break; }
    }
    for (int k = 1; k < height && sorted; k++) if (!(cdfY[k] >= cdfY[k - 1])) sorted = false;
    c->guide_ok = false;
    if (sorted) {
        HIPCHK(c, c->pr_guidex.reserve((size_t)height * (width + 2) * 4));
        HIPCHK(c, c->pr_guidey.reserve((size_t)(height + 2) * 4));
        fovpt_launch_build_guide(c->stream, (const float*)c->pr_cdfx.p, width, height, (uint32_t*)c->pr_guidex.p);
        fovpt_launch_build_guide(c->stream, (const float*)c->pr_cdfy.p, height, 1, (uint32_t*)c->pr_guidey.p);
        HIPCHK(c, c->pr_rec.reserve(n * 32));
        fovpt_launch_probe_records(c->stream, n, (const float*)c->pr_cdfx.p, (const float*)c->pr_pdfx.p, (const float4*)c->pr_data.p, (float4*)c->pr_rec.p);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->guide_ok = true;
    }
    c->guide_w = width; c->guide_h = height;
    c->rows_identical = true;
    for (int row = 1; row < height && c->rows_identical; row++)
        if (memcmp(data + (size_t)row * width, data, (size_t)width * 16) || memcmp(cdfX + (size_t)row * width, cdfX, (size_t)width * 4)
            || (pdfX && memcmp(pdfX + (size_t)row * width, pdfX, (size_t)width * 4))) c->rows_identical = false;
    memset(out, 0, sizeof(*out));
    out->width = width; out->height = height;
    out->data = (fovpt_float4*)c->pr_data.p;
    out->pdfValuesX = (float*)c->pr_pdfx.p; out->cdfValuesX = (float*)c->pr_cdfx.p;
    out->pdfValuesY = (float*)c->pr_pdfy.p; out->cdfValuesY = (float*)c->pr_cdfy.p;
    if (offset) out->offset = *offset;
    return FOVPT_OK;
}

}  // namespace

// the hierarchy build_hierarchy made becomes the scene's, with its scene facts
void adopt_hierarchy(fovpt_ctx* c, const BvhBuildResult& br, float ms)
{
    c->nodes = br.nodes; c->tris = br.tris;
    c->num_tris = br.num_refs;                       // triangle RECORDS (>= the triangles when some were split into references)
    c->bvh_num_levels = br.num_levels;
    memcpy(c->bvh_levels, br.level_first, sizeof(c->bvh_levels));
    c->stats.num_bvh_nodes = br.num_nodes; c->stats.bvh_max_depth = br.max_depth;
    c->stats.bvh_bytes = br.node_bytes; c->stats.tri_bytes = br.tri_bytes; c->stats.ms_bvh_build = ms;
}

// ---- fovpt_hierarchy_cost: measurements (refit.hip) ------------------------------------------------------------------------
// The completed measurements: the newest becomes (cost_current, cost_measured), and their slots are free again.
static void take_costs(fovpt_ctx* c)
{
    bool not_ready = false;
    for (auto& S : c->cost_slot) {
        if (!S.pending) continue;
        if (hipEventQuery(S.ev) != hipSuccess) { not_ready = true; continue; }
        S.pending = false;
        if (S.update > c->cost_measured) { c->cost_current = S.rec->cost; c->cost_measured = S.update; }
    }
    if (not_ready) (void)hipGetLastError();      // (hipErrorNotReady is an answer, not an error a later check should find)
}

// A measurement of the present tree on st, as the one of update number `update`: into a free slot, whose event is recorded
// behind it.  *out: the slot, or null when every slot is still in flight (the update is then not measured).
int enqueue_cost(fovpt_ctx* c, hipStream_t st, uint64_t update, fovpt_ctx::CostSlot** out)
{
    *out = nullptr;
    take_costs(c);
    for (auto& S : c->cost_slot) {
        if (S.pending) continue;
        if (!S.rec) HIPCHK(c, hipHostMalloc((void**)&S.rec, sizeof(TreeCostRecord), hipHostMallocDefault));
        if (!S.ev) HIPCHK(c, hipEventCreateWithFlags(&S.ev, hipEventDisableTiming));
        TreeCostRecord* d_rec = nullptr;
        HIPCHK(c, hipHostGetDevicePointer((void**)&d_rec, S.rec, 0));
        fovpt_launch_tree_cost(st, c->nodes, (uint32_t)c->stats.num_bvh_nodes, (double*)c->cost_partial.p, d_rec);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(S.ev, st));
        S.pending = true; S.update = update;
        *out = &S;
        break;
    }
    return FOVPT_OK;
}

// The cost of the hierarchy just adopted (the device is idle: fovpt_set_scene and a rebuild synchronise): cost_built, and
// cost_current for update number cost_updates.  Outside the window ms_bvh_build times.
int measure_built(fovpt_ctx* c)
{
    HIPCHK(c, c->cost_partial.reserve(2 * sizeof(double) * (size_t)fovpt_tree_cost_blocks((uint32_t)c->stats.num_bvh_nodes)));
    fovpt_ctx::CostSlot* S = nullptr;
    CHK(enqueue_cost(c, c->shadow_stream, c->cost_updates, &S));
    if (!S) return fail(c, FOVPT_E_DEVICE, "no free cost slot on an idle device");
    HIPCHK(c, hipEventSynchronize(S->ev));
    S->pending = false;
    c->cost_built = c->cost_current = S->rec->cost;
    c->cost_measured = c->cost_updates;
    return FOVPT_OK;
}

// The passes fovpt_render ran for the frame lp describes under cfg, whole (rows 0 .. gh) and on one rank: what
// find_last_writer needs to give every pixel its writing pass and launch index; and lp's camera.  Computed on a copy: the
// caller's parameters stay as they are.  fovpt_render keeps this for the frame it issued (fovpt_ctx::rendered).
void frame_levels(const fovpt_config& cfg, const fovpt_launch_params* lp, FrameDev& fd)
{
    fovpt_launch_params L = *lp;
    PassDev P[FOVPT_MAX_PASSES];
    memset(&fd, 0, sizeof(fd));
    fd.npass = frame_passes(cfg, L, P);
    for (int p = 0; p < fd.npass; p++) { fd.pass[p] = P[p]; fd.pass[p].row0 = 0; fd.pass[p].row1 = P[p].gh; fd.pass[p].frame_pass = (uint32_t)p; }
    fd.w = L.frame.size.x; fd.h = L.frame.size.y;
    fd.cx = L.frame.c.x; fd.cy = L.frame.c.y;
    fd.world = 1; fd.tile_w = 8; fd.tile_h = 4;
    set_camera(fd, lp);
}

// Everything a DevBuf member does not own.  The device is idle: fovpt_destroy has synchronised every stream.
fovpt_ctx::~fovpt_ctx()
{
    free_scene(this);
    rb.reset();                                          // (its thread is joined: free_scene ended a background rebuild)
    for (auto& S : up_stage) {
        if (S.p) (void)hipHostFree(S.p);
        if (S.ev) (void)hipEventDestroy(S.ev);
    }
    if (ev_scene) (void)hipEventDestroy(ev_scene);
    for (auto& S : cost_slot) {
        if (S.rec) (void)hipHostFree(S.rec);
        if (S.ev) (void)hipEventDestroy(S.ev);
    }
    if (pk_stream) {                                     // (fovpt_destroy's sync_all does not know the packets' copy stream)
        (void)hipStreamSynchronize(pk_stream);
        (void)hipStreamDestroy(pk_stream);
    }
    for (PacketSlot& S : pk_slot) {
        if (S.host) (void)hipHostFree(S.host);
        if (S.ev_encoded) (void)hipEventDestroy(S.ev_encoded);
        if (S.ev_done) (void)hipEventDestroy(S.ev_done);
    }
    for (StateSet& S : engine.set) {
        for (ChainEvents& ch : S.chain)
            for (int k = 0; k <= FOVPT_MAX_ITERS; k++) {
                if (ch.shade[k]) (void)hipEventDestroy(ch.shade[k]);
                if (ch.shadow[k]) (void)hipEventDestroy(ch.shadow[k]);
            }
        if (S.ev_done) (void)hipEventDestroy(S.ev_done);
    }
    for (hipEvent_t e : engine.free_events) (void)hipEventDestroy(e);
    for (int l = 1; l < FOVPT_MAX_LANES; l++) {          // ([0] are stream and shadow_stream)
        if (engine.lane_main[l]) (void)hipStreamDestroy(engine.lane_main[l]);
        if (engine.lane_shadow[l]) (void)hipStreamDestroy(engine.lane_shadow[l]);
    }
    if (stream) (void)hipStreamDestroy(stream);
    if (shadow_stream) (void)hipStreamDestroy(shadow_stream);
}

extern "C" {

int fovpt_create(fovpt_ctx** out, int device)
{
    if (!out) return fail(nullptr, FOVPT_E_INVALID, "null out pointer");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) return fail(nullptr, FOVPT_E_DEVICE, "no HIP device found (%s)", hipGetErrorString(e));   // initOptix :317-321
    if (device < 0 || device >= n) return fail(nullptr, FOVPT_E_INVALID, "device %d out of range (%d devices)", device, n);
    e = hipSetDevice(device);
    if (e != hipSuccess) return fail(nullptr, FOVPT_E_DEVICE, "hipSetDevice: %s", hipGetErrorString(e));
    fovpt_ctx* c = new fovpt_ctx;
    c->device = device;
    c->cfg = default_config();
    memset(&c->stats, 0, sizeof(c->stats));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->num_cus = prop.multiProcessorCount;
    e = make_engine(c);
    if (e != hipSuccess) { fovpt_destroy(c); return fail(nullptr, FOVPT_E_DEVICE, "stream/event creation: %s", hipGetErrorString(e)); }
    *out = c;
    return FOVPT_OK;
}

void fovpt_destroy(fovpt_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)sync_all(c);
    drain_events(c);
    (void)fovpt_comm_destroy(c);
    delete c;
}

const char* fovpt_last_error(const fovpt_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int fovpt_set_scene(fovpt_ctx* c, const fovpt_mesh_desc* meshes, int num_meshes,
                    const fovpt_texture_desc* textures, int num_textures, uint64_t* traversable_out)
{
    if (!c) return FOVPT_E_INVALID;
    if (!meshes || num_meshes <= 0) return fail(c, FOVPT_E_INVALID, "scene needs at least one mesh");
    HIPCHK(c, hipSetDevice(c->device));
    CHK(sync_all(c));
    free_scene(c);
    CHK(post_scene_changed(c));
    take_costs(c);                                   // fovpt_hierarchy_cost: (the device is idle) no measurement of the old scene stays in flight
    c->cost_updates = c->cost_measured = 0;
    uint64_t ntri = 0;
    bool any_tc = false;
    for (int m = 0; m < num_meshes; m++) {
        const fovpt_mesh_desc& D = meshes[m];
        if (!D.vertex || !D.index) return fail(c, FOVPT_E_INVALID, "mesh %d has null vertex/index", m);
        ntri += D.num_triangles;
        if (D.texcoord && D.texture_id >= 0) any_tc = true;
        if (D.texture_id >= num_textures) return fail(c, FOVPT_E_INVALID, "mesh %d references texture %d of %d (SimplePathtracer.cpp:581-583 would index out of range)", m, D.texture_id, num_textures);
    }
    if (ntri == 0) return fail(c, FOVPT_E_INVALID, "scene has no triangles");
    // the traversal addresses 48-B triangle records and 128-B nodes with 32-bit byte offsets
    if (ntri > (1ull << 26)) return fail(c, FOVPT_E_INVALID, "too many triangles (%llu > 2^26)", (unsigned long long)ntri);
    // flatten on the host: 9 floats per triangle in global primitive order (mesh order, then index order)
    std::vector<float> flat((size_t)ntri * 9);
    std::vector<uint32_t> mesh_of((size_t)ntri);
    std::vector<float> tc(any_tc ? (size_t)ntri * 6 : 0, 0.0f);
    std::vector<MeshDev> md((size_t)num_meshes);
    c->any_catcher = 0;
    // what fovpt_update_vertices needs (host only until the first update)
    c->mesh_prim0.assign((size_t)num_meshes, 0u); c->mesh_vbase.assign((size_t)num_meshes, 0u); c->mesh_nv.assign((size_t)num_meshes, 0u);
    c->h_tri_vidx.assign((size_t)ntri * 3, 0u);
    c->h_vtx.clear();
    size_t t = 0;
    for (int m = 0; m < num_meshes; m++) {
        const fovpt_mesh_desc& D = meshes[m];
        c->mesh_prim0[m] = (uint32_t)t; c->mesh_vbase[m] = (uint32_t)(c->h_vtx.size() / 3); c->mesh_nv[m] = D.num_vertices;
        c->h_vtx.insert(c->h_vtx.end(), D.vertex, D.vertex + 3 * (size_t)D.num_vertices);
        md[m].material = D.material;
        md[m].texture_id = D.texture_id >= 0 ? D.texture_id : -1;
        md[m].has_texcoord = D.texcoord ? 1 : 0;
        if (D.material.flags & FOVPT_MATERIAL_FLAG_SHADOW_CATCHER) c->any_catcher = 1;
        for (uint32_t k = 0; k < D.num_triangles; k++, t++) {
            for (int v = 0; v < 3; v++) {
                const uint32_t idx = D.index[3 * (size_t)k + v];
                if (idx >= D.num_vertices) return fail(c, FOVPT_E_INVALID, "mesh %d triangle %u indexes vertex %u of %u", m, k, idx, D.num_vertices);
                c->h_tri_vidx[t * 3 + v] = c->mesh_vbase[m] + idx;
                flat[t * 9 + v * 3 + 0] = D.vertex[3 * (size_t)idx + 0];
                flat[t * 9 + v * 3 + 1] = D.vertex[3 * (size_t)idx + 1];
                flat[t * 9 + v * 3 + 2] = D.vertex[3 * (size_t)idx + 2];
                if (any_tc && D.texcoord) { tc[t * 6 + v * 2] = D.texcoord[2 * (size_t)idx]; tc[t * 6 + v * 2 + 1] = D.texcoord[2 * (size_t)idx + 1]; }
            }
            mesh_of[t] = (uint32_t)m;
        }
    }
    DevBuf t_flat, t_mesh_of;
    HIPCHK(c, t_flat.reserve(flat.size() * 4));
    HIPCHK(c, t_mesh_of.reserve(mesh_of.size() * 4));
    float* d_flat = (float*)t_flat.p; uint32_t* d_mesh_of = (uint32_t*)t_mesh_of.p;
    HIPCHK(c, hipMemcpy(d_flat, flat.data(), flat.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_mesh_of, mesh_of.data(), mesh_of.size() * 4, hipMemcpyHostToDevice));
    if (any_tc) {
        HIPCHK(c, c->tri_tc.reserve(tc.size() * 4));
        HIPCHK(c, hipMemcpy(c->tri_tc.p, tc.data(), tc.size() * 4, hipMemcpyHostToDevice));
    }
    // textures: createTextures :748-799 (RGBA8, wrap, bilinear, normalized float)
    std::vector<TexDev> td((size_t)(num_textures > 0 ? num_textures : 1));
    for (int k = 0; k < num_textures; k++) {
        const fovpt_texture_desc& X = textures[k];
        if (!X.pixel || X.width <= 0 || X.height <= 0) return fail(c, FOVPT_E_INVALID, "texture %d is empty", k);
        void* px = nullptr;
        const size_t nb = (size_t)X.width * X.height * 4;
        HIPCHK(c, hipMalloc(&px, nb));
        c->tex_pixels.push_back(px);
        HIPCHK(c, hipMemcpy(px, X.pixel, nb, hipMemcpyHostToDevice));
        td[k].px = (const uint32_t*)px; td[k].w = X.width; td[k].h = X.height;
    }
    HIPCHK(c, c->textures.reserve(td.size() * sizeof(TexDev)));
    HIPCHK(c, hipMemcpy(c->textures.p, td.data(), td.size() * sizeof(TexDev), hipMemcpyHostToDevice));
    for (int m = 0; m < num_meshes; m++) {
        md[m].tex.px = nullptr; md[m].tex.w = md[m].tex.h = 0;
        if (md[m].texture_id >= 0) md[m].tex = td[md[m].texture_id];
    }
    HIPCHK(c, c->meshes.reserve(md.size() * sizeof(MeshDev)));
    HIPCHK(c, hipMemcpy(c->meshes.p, md.data(), md.size() * sizeof(MeshDev), hipMemcpyHostToDevice));

    BvhBuildResult br;
    float ms = 0.f;
    CHK(build_hierarchy(c, c->stream, d_flat, d_mesh_of, (uint32_t)ntri, br, ms));
    adopt_hierarchy(c, br, ms);
    c->stats.num_triangles = ntri;
    c->has_scene = true;
    c->scene_id = (c->scene_id & 0xffffffffull) + 1;
    c->scene_id |= 0x464f565000000000ull;          // 'FOVP' tag so a stale/foreign handle is recognisable
    if (traversable_out) *traversable_out = c->scene_id;
    return measure_built(c);
}

int fovpt_hierarchy_cost(fovpt_ctx* c, int flags, fovpt_hierarchy_cost_info* out)
{
    if (!c) return FOVPT_E_INVALID;
    if (!out) return fail(c, FOVPT_E_INVALID, "fovpt_hierarchy_cost: null out pointer");
    if (flags & ~FOVPT_COST_WAIT) return fail(c, FOVPT_E_INVALID, "fovpt_hierarchy_cost: unknown flag bits %d", flags);
    if (!c->has_scene) return fail(c, FOVPT_E_NO_SCENE, "fovpt_hierarchy_cost without a scene");
    HIPCHK(c, hipSetDevice(c->device));
    const bool wait = (flags & FOVPT_COST_WAIT) != 0, first = !c->cost_watching;
    c->cost_watching = true;                               // from now on every refit is followed by a measurement
    take_costs(c);
    if (c->cost_measured != c->cost_updates && (wait || first)) {
        // the present tree's measurement: the one already in flight, else a new one (refits made before watching began)
        fovpt_ctx::CostSlot* S = nullptr;
        for (auto& X : c->cost_slot)
            if (X.pending && X.update == c->cost_updates) S = &X;
        if (!S) CHK(enqueue_cost(c, c->shadow_stream, c->cost_updates, &S));
        if (!S && wait) {
            // every slot is in flight with an older tree's measurement: one of them first
            HIPCHK(c, hipEventSynchronize(c->cost_slot[0].ev));
            CHK(enqueue_cost(c, c->shadow_stream, c->cost_updates, &S));
            if (!S) return fail(c, FOVPT_E_DEVICE, "fovpt_hierarchy_cost: no free slot behind a completed measurement");
        }
        if (wait) { HIPCHK(c, hipEventSynchronize(S->ev)); take_costs(c); }
    }
    out->built = c->cost_built; out->current = c->cost_current;
    out->updates = c->cost_updates; out->measured = c->cost_measured;
    return FOVPT_OK;
}

int fovpt_set_probe(fovpt_ctx* c, int width, int height, const fovpt_float4* data,
                    const float* pdfX, const float* cdfX, const float* pdfY, const float* cdfY,
                    const fovpt_float3* offset, fovpt_probe* out)
{
    if (!c) return FOVPT_E_INVALID;
    if (!data || !pdfX || !cdfX || !pdfY || !cdfY || width <= 0 || height <= 0 || !out)
        return fail(c, FOVPT_E_INVALID, "Probe Data is not valid");                         // Probe.h:104-105
    HIPCHK(c, hipSetDevice(c->device));
    CHK(sync_all(c));
    const size_t n = (size_t)width * height;
    CHK(reserve_probe(c, width, height));
    HIPCHK(c, hipMemcpy(c->pr_pdfx.p, pdfX, n * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->pr_cdfx.p, cdfX, n * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->pr_pdfy.p, pdfY, (size_t)height * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->pr_cdfy.p, cdfY, (size_t)height * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->pr_data.p, data, n * 16, hipMemcpyHostToDevice));
    return finish_probe(c, width, height, data, pdfX, cdfX, cdfY, offset, out);
}

int fovpt_set_probe_data(fovpt_ctx* c, int width, int height, const fovpt_float4* data, const fovpt_float3* offset, fovpt_probe* out)
{
    if (!c) return FOVPT_E_INVALID;
    if (!data || width <= 0 || height <= 0 || !out) return fail(c, FOVPT_E_INVALID, "Probe Data is not valid");
    HIPCHK(c, hipSetDevice(c->device));
    CHK(sync_all(c));
    const size_t n = (size_t)width * height;
    CHK(reserve_probe(c, width, height));
    HIPCHK(c, hipMemcpy(c->pr_data.p, data, n * 16, hipMemcpyHostToDevice));
    DevBuf row_total;
    HIPCHK(c, row_total.reserve((size_t)height * 4));
    fovpt_launch_build_cdf(c->stream, width, height, (const float4*)c->pr_data.p, (float*)c->pr_pdfx.p, (float*)c->pr_cdfx.p,
                           (float*)c->pr_pdfy.p, (float*)c->pr_cdfy.p, (float*)row_total.p);
    // monotonicity decides whether the guide tables may be used; check on the host copy of the result
    std::vector<float> hx(n), hy((size_t)height);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    row_total.release();
    HIPCHK(c, hipMemcpy(hx.data(), c->pr_cdfx.p, n * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(hy.data(), c->pr_cdfy.p, (size_t)height * 4, hipMemcpyDeviceToHost));
    // (identical texel rows give identical pdfX rows: the same arithmetic on the same inputs, so none to compare here)
    return finish_probe(c, width, height, data, nullptr, hx.data(), hy.data(), offset, out);
}

int fovpt_resize(fovpt_ctx* c, int width, int height, fovpt_frame_ptrs* out)
{
    if (!c) return FOVPT_E_INVALID;
    if (width == 0 || height == 0) return FOVPT_OK;                                          // :231
    if (width < 0 || height < 0 || !out) return fail(c, FOVPT_E_INVALID, "bad resize arguments");
    HIPCHK(c, hipSetDevice(c->device));
    CHK(sync_all(c));
    const size_t n = (size_t)width * height;
    HIPCHK(c, c->fb_frame.reserve(n * 4)); HIPCHK(c, c->fb_accum.reserve(n * 16));
    HIPCHK(c, c->fb_color.reserve(n * 16)); HIPCHK(c, c->fb_normal.reserve(n * 16)); HIPCHK(c, c->fb_albedo.reserve(n * 16));
    HIPCHK(c, hipMemset(c->fb_frame.p, 0, n * 4));
    HIPCHK(c, hipMemset(c->fb_accum.p, 0, n * 16));
    HIPCHK(c, hipMemset(c->fb_color.p, 0, n * 16));
    HIPCHK(c, hipMemset(c->fb_normal.p, 0, n * 16));
    HIPCHK(c, hipMemset(c->fb_albedo.p, 0, n * 16));
    CHK(post_resize(c, width, height));                                                       // the post-frame stages follow the frame
    out->frame_buffer = (uint32_t*)c->fb_frame.p; out->accum_buffer = (fovpt_float4*)c->fb_accum.p;
    out->color_buffer = (fovpt_float4*)c->fb_color.p; out->normal_buffer = (fovpt_float4*)c->fb_normal.p;
    out->albedo_buffer = (fovpt_float4*)c->fb_albedo.p;
    return FOVPT_OK;
}

int fovpt_get_config(const fovpt_ctx* c, fovpt_config* out)
{
    if (!c || !out) return FOVPT_E_INVALID;
    *out = c->cfg;
    return FOVPT_OK;
}

int fovpt_set_config(fovpt_ctx* c, const fovpt_config* cfg)
{
    if (!c || !cfg) return FOVPT_E_INVALID;
    if (cfg->max_depth < 1 || cfg->max_depth > 32) return fail(c, FOVPT_E_INVALID, "max_depth must be in [1,32]");
    if (cfg->world < 1 || cfg->rank < 0 || cfg->rank >= cfg->world) return fail(c, FOVPT_E_INVALID, "bad rank/world %d/%d", cfg->rank, cfg->world);
    if (cfg->spp_periphery < 1 || cfg->spp_middle < 1 || cfg->spp_fovea < 1 || cfg->spp_uniform < 1) return fail(c, FOVPT_E_INVALID, "spp must be >= 1");
    if (cfg->r_inner < 0 || cfg->r_outer < cfg->r_inner) return fail(c, FOVPT_E_INVALID, "bad radii");
    if (cfg->frames_in_flight < 0 || cfg->frames_in_flight > FOVPT_MAX_LANES) return fail(c, FOVPT_E_INVALID, "frames_in_flight must be 0 (the default) or 1 .. %d (more than the context's stream pairs, FOVPT_LANES, means all of them)", FOVPT_MAX_LANES);
    if (cfg->chains_per_frame < 0 || cfg->chains_per_frame > 2) return fail(c, FOVPT_E_INVALID, "chains_per_frame must be 0, 1 or 2");
    if (cfg->options & ~(FOVPT_OPT_SKY_MISS | FOVPT_OPT_RUSSIAN_ROULETTE)) return fail(c, FOVPT_E_INVALID, "unknown option bits %d", cfg->options);
    c->cfg = *cfg;
    return FOVPT_OK;
}

int fovpt_launch(fovpt_ctx* c, const fovpt_launch_params* lp, uint32_t width, uint32_t height)
{
    if (!c || !lp) return FOVPT_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    PassDev P = pass_from_lp(lp, width, height);
    return run_passes(c, lp, &P, 1, 0);
}

int fovpt_render(fovpt_ctx* c, fovpt_launch_params* lp)
{
    if (!c || !lp) return FOVPT_E_INVALID;
    if (lp->frame.size.x == 0) return FOVPT_OK;                                              // :81-82
    HIPCHK(c, hipSetDevice(c->device));
    PassDev P[3];
    const uint32_t temp_frame = c->cfg.uniform ? 0u : lp->frame.subframe_index;              // :97 / :161 (FOV_OFF zeroes it first, :87)
    const int npass = frame_passes(c->cfg, *lp, P);
    const int rc = run_passes(c, lp, P, npass, 1);
    lp->frame.subframe_index = temp_frame;                                                   // :128-129 / :210-211
    lp->frame.subframe_index++;
    c->seq_frame = ++c->seq;                                                                  // fovpt_warp_motion: the last trace is an earlier frame's
    if (rc == FOVPT_OK) {                                                                     // what post-processing may filter
        c->rendered.w = lp->frame.size.x; c->rendered.h = lp->frame.size.y;
        frame_levels(c->cfg, lp, c->rendered.frame);
        c->rendered.uniform = c->cfg.uniform;
        c->rendered.guides = c->cfg.write_guides;
        c->rendered.world = c->cfg.world;
    }
    return rc;
}

int fovpt_synchronize(fovpt_ctx* c)
{
    if (!c) return FOVPT_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    CHK(sync_all(c));
    return FOVPT_OK;
}

int fovpt_download(fovpt_ctx* c, const void* device_src, void* host_dst, size_t n_bytes)
{
    if (!c || !device_src || !host_dst) return FOVPT_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    CHK(sync_all(c));
    HIPCHK(c, hipMemcpy(host_dst, device_src, n_bytes, hipMemcpyDeviceToHost));
    return FOVPT_OK;
}

int fovpt_get_stats(fovpt_ctx* c, fovpt_stats* out)
{
    if (!c || !out) return FOVPT_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    CHK(sync_all(c));
    drain_events(c);
    c->stats.radiance_rays = c->stats.shadow_rays = c->stats.paths = 0;
    for (StateSet& S : c->engine.set) {
        if (!S.counters.p) continue;
        unsigned long long h[3];                          // stat_radiance, stat_shadow, stat_paths
        HIPCHK(c, hipMemcpy(h, (const char*)S.counters.p + offsetof(Counters, stat_radiance), sizeof(h), hipMemcpyDeviceToHost));
        c->stats.radiance_rays += h[0]; c->stats.shadow_rays += h[1]; c->stats.paths += h[2];
    }
    *out = c->stats;
    return FOVPT_OK;
}

int fovpt_reset_stats(fovpt_ctx* c)
{
    if (!c) return FOVPT_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    CHK(sync_all(c));
    drain_events(c);
    for (StateSet& S : c->engine.set)
        if (S.counters.p) HIPCHK(c, hipMemset((char*)S.counters.p + offsetof(Counters, stat_radiance), 0, sizeof(Counters) - offsetof(Counters, stat_radiance)));
    c->stats.radiance_rays = c->stats.shadow_rays = c->stats.paths = c->stats.frames = 0;
    c->stats.ms_generate = c->stats.ms_trace = c->stats.ms_shade = c->stats.ms_shadow = c->stats.ms_resolve = 0.0;
    c->stats.n_trace_launches = c->stats.n_shadow_launches = 0;
    return FOVPT_OK;
}

// The stream on which frames COMPLETE, in order (occlusion rays and the resolve run on it): work a
// caller queues on it after fovpt_render sees the finished frame and runs before the next frame's
// resolve touches the render target.  (The head of a frame runs on an internal higher-priority stream.)
void* fovpt_stream(fovpt_ctx* c) { return c ? (void*)c->shadow_stream : nullptr; }

// ---- host helpers ------------------------------------------------------------------------
// ProbeData::BuildCDF, PT_sv5_/Probe.h:29-77.  Strictly sequential fp32 sums: the order is part of
// the result.
int fovpt_probe_build_cdf(int width, int height, const fovpt_float4* data,
                          float* pdfValuesX, float* cdfValuesX, float* pdfValuesY, float* cdfValuesY)
{
    if (width <= 0 || height <= 0 || !data || !pdfValuesX || !cdfValuesX || !pdfValuesY || !cdfValuesY) return FOVPT_E_INVALID;
    volatile float col_total = 0.0f;                  // volatile: keep every partial sum rounded to fp32
    for (int row = 0; row < height; ++row) {
        volatile float row_total = 0.0f;
        float* pdf_row = pdfValuesX + (size_t)row * width;
        float* cdf_row = cdfValuesX + (size_t)row * width;
        const fovpt_float4* px = data + (size_t)row * width;
        for (int k = 0; k < width; ++k) {
            const float lum = px[k].x * 0.3f + px[k].y * 0.6f + px[k].z * 0.1f;   // Luminance, maths.h:165-168
            row_total = row_total + lum;
            pdf_row[k] = lum;
            cdf_row[k] = row_total;
        }
        const float inv = 1.0f / row_total;
        for (int k = 0; k < width; ++k) { pdf_row[k] *= inv; cdf_row[k] *= inv; }
        col_total = col_total + row_total;
        pdfValuesY[row] = row_total;
        cdfValuesY[row] = col_total;
    }
    const float total = col_total;
    for (int row = 0; row < height; ++row) { cdfValuesY[row] /= total; pdfValuesY[row] /= total; }
    return FOVPT_OK;
}

// sutil::Camera::UVWFrame, sutil/Camera.cpp:32-44
int fovpt_camera_uvw(const fovpt_float3* eye, const fovpt_float3* lookat, const fovpt_float3* up,
                     float fovY, float aspect, fovpt_float3* U, fovpt_float3* V, fovpt_float3* W)
{
    if (!eye || !lookat || !up || !U || !V || !W) return FOVPT_E_INVALID;
    const float wx = lookat->x - eye->x, wy = lookat->y - eye->y, wz = lookat->z - eye->z;
    const float wlen = sqrtf(wx * wx + wy * wy + wz * wz);
    float ux = wy * up->z - wz * up->y, uy = wz * up->x - wx * up->z, uz = wx * up->y - wy * up->x;    // cross(W, up)
    float inv = 1.0f / sqrtf(ux * ux + uy * uy + uz * uz);
    ux *= inv; uy *= inv; uz *= inv;
    float vx = uy * wz - uz * wy, vy = uz * wx - ux * wz, vz = ux * wy - uy * wx;                      // cross(U, W)
    inv = 1.0f / sqrtf(vx * vx + vy * vy + vz * vz);
    vx *= inv; vy *= inv; vz *= inv;
    const float vlen = wlen * tanf(0.5f * fovY * 3.14159265358979323846f / 180.0f);
    vx *= vlen; vy *= vlen; vz *= vlen;
    const float ulen = vlen * aspect;
    ux *= ulen; uy *= ulen; uz *= ulen;
    U->x = ux; U->y = uy; U->z = uz; V->x = vx; V->y = vy; V->z = vz; W->x = wx; W->y = wy; W->z = wz;
    return FOVPT_OK;
}

}  // extern "C"
