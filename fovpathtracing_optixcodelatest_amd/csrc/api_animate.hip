// api_animate.hip -- animated geometry over the C ABI (include/fovpt.h; kernels: refit.hip): fovpt_update_vertices,
// fovpt_update_transforms, fovpt_set_skins / fovpt_update_skinned, fovpt_set_morphs / fovpt_update_morphed, fovpt_set_rig /
// fovpt_update_animated (kernel: rig.hip).
//
// Every entry point validates all of its arguments first (all or nothing; Listed is the part they share).  What fovpt_set_skins,
// fovpt_set_morphs and fovpt_set_rig accept and how they lay their data out, and the overflow rules of the update calls, are
// fovpt_animplan.h's: pure host functions of the caller's description and an AnimScene, tested without a GPU.  This file keeps what
// needs a context or a device: the set-up calls reserve, upload and commit an accepted plan (replace_buffers).  An update is then
// three steps on fovpt_stream(), the stream every job's resolve, and so every job's last traversal launch, is ordered on:
// begin_update (what has to happen ahead of any new position), the source's own write_* (the new positions into up_vtx) and
// finish_update (the refit, with the event the next job waits for, or the rebuild).  A new source is a new write_*.
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "fovpt_ctx.h"

namespace {

// A refused plan or overflow check of fovpt_animplan.h: its code and its text to the context
int refused(fovpt_ctx* c, const AnimVerdict& V) { return fail(c, V.code, "%s", V.text.c_str()); }

// What the plan functions read of the scene and of the skins and morphs it has now
AnimScene anim_scene(const fovpt_ctx* c)
{
    AnimScene sc;
    sc.mesh.resize(c->mesh_nv.size());
    for (size_t m = 0; m < sc.mesh.size(); m++) {
        AnimMesh& M = sc.mesh[m];
        M.nv = c->mesh_nv[m];
        if (!c->skins.empty()) { M.skin_joints = c->skins[m].num_joints; M.pal_first = c->skins[m].pal_first; }
        if (!c->morphs.empty()) { M.morph_targets = c->morphs[m].num_targets; M.morph_entries = c->morphs[m].ent.size(); M.w_first = c->morphs[m].w_first; }
    }
    return sc;
}

// What the entry points check first, in this order: open() the context, the scene, the count and the array (`what`: the
// caller's word for its entries) and the flags (flag_text: the caller's wording); then mesh(), entry by entry between the
// caller's own checks, that the mesh exists and is not listed twice (check(); mesh() also adds it to `meshes`, the list an update
// goes on with).
struct Listed {
    fovpt_ctx* c = nullptr; const char* who = nullptr; int nmesh = 0;
    std::vector<char> seen; std::vector<int> meshes;
    int open(fovpt_ctx* c_, const char* who_, int num, const void* at, const char* what, int flags = 0, int allowed = 0,
             const char* flag_text = "%s: unknown flag bits %d")
    {
        if (!c_) return FOVPT_E_INVALID;
        c = c_; who = who_; nmesh = (int)c->mesh_nv.size();
        if (!c->has_scene) return fail(c, FOVPT_E_NO_SCENE, "%s without a scene", who);
        if (num < 0 || (num > 0 && !at)) return fail(c, FOVPT_E_INVALID, "%s: %d %s at %p", who, num, what, at);
        if (flags & ~allowed) return fail(c, FOVPT_E_INVALID, flag_text, who, flags);
        if ((flags & FOVPT_UPDATE_REBUILD) && (flags & FOVPT_UPDATE_REBUILD_ASYNC))
            return fail(c, FOVPT_E_INVALID, "%s: FOVPT_UPDATE_REBUILD together with FOVPT_UPDATE_REBUILD_ASYNC", who);
        seen.assign((size_t)nmesh, 0);
        return FOVPT_OK;
    }
    int check(int m)
    {
        AnimVerdict V;
        return anim_list_mesh(V, seen, who, m) ? refused(c, V) : FOVPT_OK;
    }
    int mesh(int m) { CHK(check(m)); meshes.push_back(m); return FOVPT_OK; }      // (at most nmesh entries: none is listed twice)
};

// What every update checks of the scene once its own arguments are in order
int check_updatable(fovpt_ctx* c, const char* who)
{
    if (c->h_vtx.size() / 3 >= (1ull << 32)) return fail(c, FOVPT_E_INVALID, "%s: more than 2^32 - 1 vertices", who);
    if (c->bvh_num_levels == 0) return fail(c, FOVPT_E_INVALID, "%s: the hierarchy has more than %d levels", who, FOVPT_BVH_MAX_LEVELS);
    return FOVPT_OK;
}

// Once per scene, for the overflow rules: the largest |coordinate| of every mesh's rest positions
void ensure_absmax(fovpt_ctx* c)
{
    if (!c->mesh_absmax.empty()) return;
    const int nmesh = (int)c->mesh_nv.size();
    c->mesh_absmax.assign((size_t)nmesh, 0.0);
    for (int m = 0; m < nmesh; m++) {
        const float* v = c->h_vtx.data() + 3 * (size_t)c->mesh_vbase[m];
        for (size_t i = 0; i < 3 * (size_t)c->mesh_nv[m]; i++) c->mesh_absmax[m] = std::fmax(c->mesh_absmax[m], std::fabs((double)v[i]));
    }
}

// One of refit.hip's batch structs (up to FOVPT_GATHER_BATCH meshes per launch) and what launches it.  put(): a new entry of n
// vertices, whose other members fill(g, i) sets; true when the batch is now full.  flush(): launches what the batch holds, if
// anything.  add(): put, and flush when full.  So add() per entry and one flush() behind the list launch every entry once, in
// order, and never an empty batch.
template <class B, class Launch>
struct Batch {
    B g; Launch launch;
    explicit Batch(Launch l) : launch(l) { memset(&g, 0, sizeof(g)); }
    template <class Fill> bool put(uint32_t n, Fill fill)
    {
        fill(g, g.count);
        g.n[g.count] = n; g.max_n = n > g.max_n ? n : g.max_n;
        return ++g.count == FOVPT_GATHER_BATCH;
    }
    void flush() { if (g.count) { launch(g); memset(&g, 0, sizeof(g)); } }
    template <class Fill> void add(uint32_t n, Fill fill) { if (put(n, fill)) flush(); }
};
template <class B, class Launch> Batch<B, Launch> batch_of(Launch l) { return Batch<B, Launch>(l); }

// The next of the two pinned staging buffers, with room for `bytes`, once the copies it last fed have run
int take_stage(fovpt_ctx* c, size_t bytes, fovpt_ctx::Staging** out)
{
    auto& S = c->up_stage[c->up_next];
    c->up_next ^= 1;
    if (S.pending) { HIPCHK(c, hipEventSynchronize(S.ev)); S.pending = false; }      // its previous copy has run
    if (S.bytes < bytes) {
        if (S.p) (void)hipHostFree(S.p);
        S.p = nullptr; S.bytes = 0;
        HIPCHK(c, hipHostMalloc(&S.p, bytes, hipHostMallocDefault));
        S.bytes = bytes;
    }
    *out = &S;
    return FOVPT_OK;
}

// The host data of one call on its way to the device.  open(): a staging buffer for all of it, `floats` in all.  The data goes into
// the buffer in call order and from there to its place, on fovpt_stream(): send() one piece; runs() the pieces of a list in units
// of `stride` floats of dst, neighbours in one copy (a run goes on while the next entry's place follows directly).  done(): the
// buffer's event behind the copies, once per call.
struct Piece { const float* src; uint32_t place, count; };      // count 0: the entry has none
struct Stage {
    fovpt_ctx* c; fovpt_ctx::Staging* S; float* h;
    int open(size_t floats) { CHK(take_stage(c, floats * 4, &S)); h = (float*)S->p; return FOVPT_OK; }
    int send(float* dst, const float* src, size_t floats)
    {
        memcpy(h, src, floats * 4);
        HIPCHK(c, hipMemcpyAsync(dst, h, floats * 4, hipMemcpyHostToDevice, c->shadow_stream));
        h += floats;
        return FOVPT_OK;
    }
    template <class Get> int runs(int num, Get piece, float* dst, size_t stride)
    {
        for (int k = 0; k < num;) {
            Piece p = piece(k);
            if (!p.count) { k++; continue; }
            float* run = h;
            const uint32_t first = p.place;
            size_t n = 0;
            do {
                memcpy(h, p.src, 4 * stride * p.count);
                h += stride * p.count; n += p.count;
            } while (++k < num && (p = piece(k)).count && p.place == first + n);
            HIPCHK(c, hipMemcpyAsync(dst + stride * first, run, 4 * stride * n, hipMemcpyHostToDevice, c->shadow_stream));
        }
        return FOVPT_OK;
    }
    int done() { HIPCHK(c, hipEventRecord(S->ev, c->shadow_stream)); S->pending = true; return FOVPT_OK; }
};

// ---- FOVPT_UPDATE_REBUILD_ASYNC: the hierarchy built beside the frames ---------------------------------------------------------
// The slot and its transitions are fovpt_bgjob.h's.  Here: what a request puts on fovpt_stream() (start_rebuild), what the
// builder's thread does with it (run_rebuild: that function and what it calls touch no fovpt_ctx), how a finished hierarchy
// becomes the scene's without a wait (adopt_ready) and how the one it replaces goes once nothing can read it (retire_poll).
using RebuildJob = fovpt::BgJob<fovpt_ctx::RebuildDone>;
int enqueue_refit(fovpt_ctx* c);

void free_rebuild_result(fovpt_ctx::RebuildDone& d)
{
    free_hierarchy(d.br);
    if (d.partial) (void)hipFree(d.partial);
    d = fovpt_ctx::RebuildDone();
}

// Retired memory whose events have all completed is freed (hipFree waits for the device: DESIGN.md, section 27, has what that
// costs where this is called); nothing here waits for an event.
void retire_poll(fovpt_ctx* c)
{
    bool not_ready = false;
    for (size_t i = 0; i < c->retired.size();) {
        fovpt_ctx::Retired& T = c->retired[i];
        bool done = true;
        for (hipEvent_t e : T.ev)
            if (hipEventQuery(e) != hipSuccess) { done = false; break; }
        if (!done) { not_ready = true; i++; continue; }
        for (void* p : T.p) if (p) (void)hipFree(p);
        for (hipEvent_t e : T.ev) (void)hipEventDestroy(e);
        c->retired.erase(c->retired.begin() + (long)i);
    }
    if (not_ready) (void)hipGetLastError();      // (hipErrorNotReady is an answer, not an error a later check should find)
}

// The same on an idle device (the caller has synchronised every stream): everything retired goes
void retire_idle(fovpt_ctx* c)
{
    for (fovpt_ctx::Retired& T : c->retired) {
        for (void* p : T.p) if (p) (void)hipFree(p);
        for (hipEvent_t e : T.ev) (void)hipEventDestroy(e);
    }
    c->retired.clear();
}

// fovpt_set_scene, a synchronous rebuild and fovpt_destroy end a background build: its thread is joined, its result freed
void end_background_rebuild(fovpt_ctx* c)
{
    if (!c->rb) return;
    (void)c->rb->job.discard([&](fovpt_ctx::RebuildDone& d) { c->rb->ms_build = d.ms; free_rebuild_result(d); });
}

// A context's first flagged call: the builder's stream, of the lowest priority the device offers, the snapshot's event and the
// pinned record the builder's cost measurement writes
int ensure_rebuild(fovpt_ctx* c)
{
    if (c->rb) return FOVPT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    std::unique_ptr<fovpt_ctx::Rebuild> R(new fovpt_ctx::Rebuild);
    int least = 0, greatest = 0;
    HIPCHK(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIPCHK(c, hipStreamCreateWithPriority(&R->st, hipStreamNonBlocking, least));
    HIPCHK(c, hipEventCreateWithFlags(&R->ev_snapshot, hipEventDisableTiming));
    HIPCHK(c, hipHostMalloc((void**)&R->rec, sizeof(TreeCostRecord), hipHostMallocDefault));
    R->job.on_destroy(free_rebuild_result);
    c->rb = std::move(R);
    return FOVPT_OK;
}

// On the builder's thread.  build_hierarchy as fovpt_set_scene runs it, over the snapshot, on the builder's stream behind the
// snapshot's event; then what a refit needs of the result, and its cost with partial sums of its own.
int run_rebuild(fovpt_ctx::Rebuild* R, fovpt_ctx::RebuildDone& out, std::string& text)
{
    const fovpt_ctx::Rebuild::In& in = R->in;
    char err[384];
    hipError_t e = hipSuccess;
    const char* what = nullptr;
#define TRY(x) do { if (e == hipSuccess && (e = (x)) != hipSuccess) what = #x; } while (0)
    TRY(hipSetDevice(in.device));
    TRY(hipStreamWaitEvent(R->st, R->ev_snapshot, 0));
    TRY(hipMemcpyAsync(R->mesh_of.p, in.h_mesh_of.data(), 4 * (size_t)in.ntri, hipMemcpyHostToDevice, R->st));
    if (e != hipSuccess) { text = std::string(what) + ": " + hipGetErrorString(e); return FOVPT_E_DEVICE; }
    const int rc = build_hierarchy(R->st, in.sw, (const float*)R->flat.p, (const uint32_t*)R->mesh_of.p, in.ntri, out.br, out.ms, err, sizeof(err));
    if (rc) { text = err; out = fovpt_ctx::RebuildDone(); return rc; }
    if (out.br.num_levels == 0) {
        // (a refit needs the levels, and an adopted hierarchy is refitted at once)
        free_rebuild_result(out);
        snprintf(err, sizeof(err), "the hierarchy has more than %d levels", FOVPT_BVH_MAX_LEVELS);
        text = err;
        return FOVPT_E_INVALID;
    }
    out.partial_bytes = 2 * sizeof(double) * (size_t)fovpt_tree_cost_blocks(out.br.num_nodes);
    TreeCostRecord* d_rec = nullptr;
    TRY(hipMalloc(&out.partial, out.partial_bytes ? out.partial_bytes : 16));
    TRY(hipHostGetDevicePointer((void**)&d_rec, R->rec, 0));
    if (e == hipSuccess) {
        fovpt_launch_tree_cost(R->st, out.br.nodes, out.br.num_nodes, (double*)out.partial, d_rec);
        TRY(hipGetLastError());
        TRY(hipStreamSynchronize(R->st));
    }
#undef TRY
    if (e != hipSuccess) { text = std::string(what) + ": " + hipGetErrorString(e); free_rebuild_result(out); return FOVPT_E_DEVICE; }
    out.cost = R->rec->cost;
    if (in.delay_ms > 0) std::this_thread::sleep_for(std::chrono::milliseconds(in.delay_ms));      // FOVPT_ASYNC_BUILD_DELAY_MS (tests)
    return FOVPT_OK;
}

// The snapshot of the current positions on fovpt_stream(), behind whatever the call has enqueued, and the build over it.  The
// slot is idle (update() looked).  Never waits for the device.  The environment is read here, on the caller's thread.
int start_rebuild(fovpt_ctx* c)
{
    fovpt_ctx::Rebuild* R = c->rb.get();
    const hipStream_t st = c->shadow_stream;
    const uint32_t ntri = (uint32_t)c->stats.num_triangles;
    const int nmesh = (int)c->mesh_nv.size();
    HIPCHK(c, R->flat.reserve((size_t)ntri * 36));
    HIPCHK(c, R->mesh_of.reserve((size_t)ntri * 4));
    if (R->in.h_mesh_of.size() != ntri) {
        R->in.h_mesh_of.resize(ntri);
        for (int m = 0; m < nmesh; m++) {
            const uint32_t end = m + 1 < nmesh ? c->mesh_prim0[m + 1] : ntri;
            for (uint32_t t = c->mesh_prim0[m]; t < end; t++) R->in.h_mesh_of[t] = (uint32_t)m;
        }
    }
    fovpt_launch_flatten(st, ntri, (const uint3*)c->up_vidx.p, (const float*)c->up_vtx.p, (float*)R->flat.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(R->ev_snapshot, st));
    R->in.device = c->device;
    R->in.ntri = ntri;
    R->in.sw = fovpt_bvh_switches();
    const char* delay = getenv("FOVPT_ASYNC_BUILD_DELAY_MS");
    R->in.delay_ms = delay ? atoi(delay) : 0;
    R->snapshot_update = c->cost_updates;
    (void)R->job.request([R](fovpt_ctx::RebuildDone& out, std::string& text) { return run_rebuild(R, out, text); });
    return FOVPT_OK;
}

// READY: the finished hierarchy becomes the scene's, on fovpt_stream() and without a wait.  Frames already issued keep the old
// one in their kernel arguments (nothing on the device holds a copy of the scene's pointers): it is retired with an event behind
// everything enqueued so far on every stream that traces, and so are the partial sums a cost measurement in flight may use; the
// builder's own become the context's, sized for the new tree.  Then a refit over the CURRENT positions -- the snapshot may be
// several updates old -- with the event the next job waits for, counted as one update.  Any other state: nothing.
int adopt_ready(fovpt_ctx* c)
{
    fovpt_ctx::Rebuild* R = c->rb.get();
    if (!R || R->job.state() != RebuildJob::READY) return FOVPT_OK;
    fovpt_ctx::Retired T;
    T.p[0] = c->nodes; T.p[1] = c->cost_partial.p;
    hipError_t e = hipSuccess;
    auto behind = [&](hipStream_t s) {
        hipEvent_t ev = nullptr;
        if (!s || e != hipSuccess || (e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return;
        T.ev.push_back(ev);
        e = hipEventRecord(ev, s);
    };
    behind(c->shadow_stream);
    for (int k = 0; k < c->engine.num_trace_streams; k++) behind(c->engine.trace_stream[k]);
    if (e != hipSuccess) {
        // nothing has changed yet: the old hierarchy stays, the new one waits for the next call
        for (hipEvent_t ev : T.ev) (void)hipEventDestroy(ev);
        return fail(c, FOVPT_E_DEVICE, "adopting the rebuilt hierarchy: %s", hipGetErrorString(e));
    }
    fovpt_ctx::RebuildDone D;
    (void)R->job.adopt(&D);
    c->retired.push_back(T);
    c->cost_partial.p = D.partial; c->cost_partial.bytes = D.partial_bytes ? D.partial_bytes : 16;
    adopt_hierarchy(c, D.br, D.ms);
    R->ms_build = D.ms;
    c->cost_built = D.cost;
    c->seq_adopt = ++c->seq;                           // fovpt_warp_motion: hit records traced before address the old triangle records
    return enqueue_refit(c);
}

// ---- the three steps of an update -----------------------------------------------------------------------------------------
// Ahead of the new positions of the listed meshes: a rebuild waits for the device; the scene's first update makes the device
// copies of what fovpt_set_scene kept; fovpt_temporal_motion's tracking copies the positions about to be overwritten; from_rest
// (the source reads the rest positions: its caller passed an array, if an empty one): the scene's first puts them on the device.
// The scene's first update: the device copies of what fovpt_set_scene kept, ordered on fovpt_stream() like everything an update does
int ensure_device_copies(fovpt_ctx* c)
{
    if (c->up_vtx.p) return FOVPT_OK;
    const hipStream_t st = c->shadow_stream;
    if (!c->ev_scene) HIPCHK(c, hipEventCreateWithFlags(&c->ev_scene, hipEventDisableTiming));
    for (auto& S : c->up_stage)
        if (!S.ev) HIPCHK(c, hipEventCreateWithFlags(&S.ev, hipEventDisableTiming));
    HIPCHK(c, c->up_vidx.reserve(c->h_tri_vidx.size() * 4));
    HIPCHK(c, c->up_vtx.reserve(c->h_vtx.size() * 4));
    HIPCHK(c, hipMemcpyAsync(c->up_vidx.p, c->h_tri_vidx.data(), c->h_tri_vidx.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->up_vtx.p, c->h_vtx.data(), c->h_vtx.size() * 4, hipMemcpyHostToDevice, st));
    return FOVPT_OK;
}

int begin_update(fovpt_ctx* c, const std::vector<int>& meshes, bool rebuild, bool from_rest)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (rebuild) {
        CHK(sync_all(c));
        end_background_rebuild(c);                     // a synchronous rebuild ends a background one: joined, its result discarded
        retire_idle(c);
    }
    c->seq_update = ++c->seq;                          // fovpt_warp_motion: the last temporal step and trace are of the geometry before
    const hipStream_t st = c->shadow_stream;
    CHK(ensure_device_copies(c));
    if (!c->tm_tracking) c->tm_untracked = c->tm_untracked || !meshes.empty();
    else {
        // fovpt_temporal_motion's previous positions: what a mesh holds now, ahead of the interval's first overwrite of it
        HIPCHK(c, c->vtx_prev.reserve(c->h_vtx.size() * 4));
        auto b = batch_of<VertexTrack>([&](const VertexTrack& g) {
            fovpt_launch_gather_vertices_prev(st, g, (const float*)c->up_vtx.p, (float*)c->vtx_prev.p, (uint64_t*)c->tm_mark.p, c->tm_epoch);
        });
        for (const int mesh : meshes) {
            if (c->tm_mesh_epoch[mesh] == c->tm_epoch) continue;
            c->tm_mesh_epoch[mesh] = c->tm_epoch;
            b.add(c->mesh_nv[mesh], [&](VertexTrack& g, int i) { g.first[i] = c->mesh_vbase[mesh]; g.mesh[i] = (uint32_t)mesh; });
        }
        b.flush();
        HIPCHK(c, hipGetLastError());
    }
    if (from_rest && !c->rest_vtx.p) {
        // the first transforms or poses of the scene: the rest positions stay on the device
        HIPCHK(c, c->rest_vtx.reserve(c->h_vtx.size() * 4));
        HIPCHK(c, hipMemcpyAsync(c->rest_vtx.p, c->h_vtx.data(), c->h_vtx.size() * 4, hipMemcpyHostToDevice, st));
    }
    return FOVPT_OK;
}

// Behind the new positions: the refit, enqueued on the same stream, with the event the next job waits for (and the tree's cost
// behind it when fovpt_hierarchy_cost is watching); or FOVPT_UPDATE_REBUILD, fovpt_set_scene's build over the current vertices
// (the old hierarchy stays if it fails).
int enqueue_refit(fovpt_ctx* c)
{
    const hipStream_t st = c->shadow_stream;
    fovpt_launch_refit(st, c->nodes, c->tris, c->bvh_levels, c->bvh_num_levels, (const uint3*)c->up_vidx.p, (const float*)c->up_vtx.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_scene, st));
    c->engine.refit_pending = true;
    c->cost_updates++;
    fovpt_ctx::CostSlot* S = nullptr;
    return c->cost_watching ? enqueue_cost(c, st, c->cost_updates, &S) : FOVPT_OK;
}

int finish_update(fovpt_ctx* c, bool rebuild)
{
    const hipStream_t st = c->shadow_stream;
    const float* vtx = (const float*)c->up_vtx.p;
    if (!rebuild) return enqueue_refit(c);
    const int nmesh = (int)c->mesh_nv.size();
    const uint32_t ntri = (uint32_t)c->stats.num_triangles;
    DevBuf t_flat, t_mesh_of;
    HIPCHK(c, t_flat.reserve((size_t)ntri * 36));
    HIPCHK(c, t_mesh_of.reserve((size_t)ntri * 4));
    std::vector<uint32_t> mesh_of((size_t)ntri);
    for (int m = 0; m < nmesh; m++) {
        const uint32_t end = m + 1 < nmesh ? c->mesh_prim0[m + 1] : ntri;
        for (uint32_t t = c->mesh_prim0[m]; t < end; t++) mesh_of[t] = (uint32_t)m;
    }
    HIPCHK(c, hipMemcpyAsync(t_mesh_of.p, mesh_of.data(), mesh_of.size() * 4, hipMemcpyHostToDevice, st));
    fovpt_launch_flatten(st, ntri, (const uint3*)c->up_vidx.p, vtx, (float*)t_flat.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));
    BvhBuildResult br;
    float ms = 0.f;
    CHK(build_hierarchy(c, st, (const float*)t_flat.p, (const uint32_t*)t_mesh_of.p, ntri, br, ms));
    (void)hipFree(c->nodes);                           // (the device is idle: begin_update's sync_all, and the build synchronised)
    adopt_hierarchy(c, br, ms);
    c->cost_updates++;
    return measure_built(c);
}

// What the update calls do once everything is validated.  With FOVPT_UPDATE_REBUILD_ASYNC the call is the one without the flag;
// `start` (the slot was idle when the call came in) then adds the snapshot and the background build behind it.
template <class Write> int update(const Listed& L, int flags, bool from_rest, Write write)
{
    fovpt_ctx* c = L.c;
    const bool rebuild = (flags & FOVPT_UPDATE_REBUILD) != 0;
    CHK(check_updatable(c, L.who));
    bool start = false;
    if (flags & FOVPT_UPDATE_REBUILD_ASYNC) {
        CHK(ensure_rebuild(c));
        start = c->rb->job.state() == fovpt::BgJob<fovpt_ctx::RebuildDone>::IDLE;
        if (!start) c->rb->job.count_ignored();
    }
    if (L.meshes.empty() && !rebuild) {
        if (!start) return FOVPT_OK;
        // a background rebuild alone: nothing moves, no refit, nothing is counted
        HIPCHK(c, hipSetDevice(c->device));
        retire_poll(c);
        CHK(ensure_device_copies(c));
        return start_rebuild(c);
    }
    if (c->rb && !rebuild) {
        HIPCHK(c, hipSetDevice(c->device));
        retire_poll(c);
        CHK(adopt_ready(c));
    }
    CHK(begin_update(c, L.meshes, rebuild, from_rest));
    CHK(write());
    CHK(finish_update(c, rebuild));
    return start ? start_rebuild(c) : FOVPT_OK;
}

// ---- the six sources: validated entries to new positions in up_vtx -------------------------------------------------------
// host arrays: through the staging buffer, one copy per mesh
int write_host(fovpt_ctx* c, const fovpt_vertex_update* up, int num, size_t floats)
{
    Stage stage{c};
    if (!floats) return FOVPT_OK;
    CHK(stage.open(floats));
    for (int k = 0; k < num; k++) CHK(stage.send((float*)c->up_vtx.p + 3 * (size_t)c->mesh_vbase[up[k].mesh], up[k].vertex, 3 * (size_t)up[k].num_vertices));
    return stage.done();
}

// device arrays: by a gather kernel
int write_device(fovpt_ctx* c, const fovpt_vertex_update* up, int num)
{
    auto b = batch_of<VertexGather>([&](const VertexGather& g) { fovpt_launch_gather_vertices(c->shadow_stream, g, (float*)c->up_vtx.p); });
    for (int k = 0; k < num; k++) b.add(up[k].num_vertices, [&](VertexGather& g, int i) { g.src[i] = up[k].vertex; g.dst[i] = c->mesh_vbase[up[k].mesh]; });
    b.flush();
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

// the rest positions through per-mesh matrices
int write_transforms(fovpt_ctx* c, const fovpt_mesh_transform* tf, int num)
{
    auto b = batch_of<VertexTransform>([&](const VertexTransform& g) { fovpt_launch_transform_vertices(c->shadow_stream, g, (const float*)c->rest_vtx.p, (float*)c->up_vtx.p); });
    for (int k = 0; k < num; k++)
        b.add(c->mesh_nv[tf[k].mesh], [&](VertexTransform& g, int i) { memcpy(g.m[i], tf[k].m, sizeof(g.m[0])); g.first[i] = c->mesh_vbase[tf[k].mesh]; });
    b.flush();
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

// the rest positions through per-vertex blends of per-mesh joint palettes: device palettes in place, host palettes (`floats` in
// all) staged to the meshes' places in skin_pal
int write_skinned(fovpt_ctx* c, const fovpt_skin_pose* poses, int num, bool device, size_t floats)
{
    Stage stage{c};
    if (!device && floats) {
        CHK(stage.open(floats));
        CHK(stage.runs(num, [&](int k) { return Piece{poses[k].matrices, c->skins[poses[k].mesh].pal_first, poses[k].num_joints}; }, (float*)c->skin_pal.p, 12));
        CHK(stage.done());
    }
    auto b = batch_of<VertexSkin>([&](const VertexSkin& g) {
        fovpt_launch_skin_vertices(c->shadow_stream, g, (const float*)c->rest_vtx.p, (const uint2*)c->skin_joints.p, (const float4*)c->skin_weights.p, (float*)c->up_vtx.p);
    });
    for (int k = 0; k < num; k++) {
        const fovpt_ctx::Skin& K = c->skins[poses[k].mesh];
        b.add(c->mesh_nv[poses[k].mesh], [&](VertexSkin& g, int i) {
            g.pal[i] = device ? poses[k].matrices : (const float*)c->skin_pal.p + 12 * (size_t)K.pal_first;
            g.first[i] = c->mesh_vbase[poses[k].mesh]; g.skin[i] = K.first;
        });
    }
    b.flush();
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

// the rest positions plus their weighted morph deltas, and through the skin where a pose has a palette: device weights and
// palettes in place, host ones (`floats` in all) staged, the weights and then the palettes, to the meshes' places in morph_w
// and skin_pal
int write_morphed(fovpt_ctx* c, const fovpt_morph_pose* poses, int num, bool device, size_t floats)
{
    Stage stage{c};
    if (!device && floats) {
        CHK(stage.open(floats));
        CHK(stage.runs(num, [&](int k) { return Piece{poses[k].weights, c->morphs[poses[k].mesh].w_first, poses[k].num_targets}; }, (float*)c->morph_w.p, 1));
        CHK(stage.runs(num, [&](int k) { return Piece{poses[k].matrices, poses[k].num_joints ? c->skins[poses[k].mesh].pal_first : 0u, poses[k].num_joints}; },
                       (float*)c->skin_pal.p, 12));
        CHK(stage.done());
    }
    // two batches side by side: the poses without a palette (k_morph_vertices) and those with one (k_morph_skin_vertices)
    const hipStream_t st = c->shadow_stream;
    const float* rest = (const float*)c->rest_vtx.p;
    const uint32_t* off = (const uint32_t*)c->morph_off.p;
    const MorphEntry* ent = (const MorphEntry*)c->morph_ent.p;
    float* vtx = (float*)c->up_vtx.p;
    auto plain = batch_of<VertexMorph>([&](const VertexMorph& g) { fovpt_launch_morph_vertices(st, g, rest, off, ent, vtx); });
    auto skinned = batch_of<VertexMorph>([&](const VertexMorph& g) {
        fovpt_launch_morph_skin_vertices(st, g, rest, off, ent, (const uint2*)c->skin_joints.p, (const float4*)c->skin_weights.p, vtx);
    });
    for (int k = 0; k < num; k++) {
        const fovpt_morph_pose& P = poses[k];
        const fovpt_ctx::Morph& M = c->morphs[P.mesh];
        auto fill = [&](VertexMorph& g, int i) {
            g.w[i] = device ? P.weights : (const float*)c->morph_w.p + M.w_first;
            g.first[i] = c->mesh_vbase[P.mesh]; g.off[i] = M.off_first;
            if (!P.num_joints) return;
            g.pal[i] = device ? P.matrices : (const float*)c->skin_pal.p + 12 * (size_t)c->skins[P.mesh].pal_first;
            g.skin[i] = c->skins[P.mesh].first;
        };
        // The order of the launches is the one this call has always had: a batch launches at the pose that fills it, except at
        // the list's last pose, where every batch that holds something launches, the one without palettes first.  So a batch
        // the last pose fills is not launched here but left to the two flushes below.
        const bool full = P.num_joints ? skinned.put(c->mesh_nv[P.mesh], fill) : plain.put(c->mesh_nv[P.mesh], fill);
        if (full && k + 1 < num) { if (P.num_joints) skinned.flush(); else plain.flush(); }
    }
    plain.flush();
    skinned.flush();
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

// a rig's clip at a time: k_rig_pose leaves the palettes in skin_pal, the weights in morph_w and the rigid matrices in the rig's
// own array, all on this stream; then every bound mesh through the batch of its kind, reading those places
int write_animated(fovpt_ctx* c, int clip, float time)
{
    const fovpt_ctx::Rig& R = c->rig;
    const hipStream_t st = c->shadow_stream;
    RigDev d = R.dev;
    d.node_chan += 3 * (size_t)d.num_nodes * (size_t)clip;
    d.w_chan += (size_t)d.num_wjobs * (size_t)clip;
    d.skin_pal = (float*)c->skin_pal.p;
    d.morph_w = (float*)c->morph_w.p;
    fovpt_launch_rig_pose(st, d, time, R.threads);
    const float* rest = (const float*)c->rest_vtx.p;
    const uint32_t* off = (const uint32_t*)c->morph_off.p;
    const MorphEntry* ent = (const MorphEntry*)c->morph_ent.p;
    const uint2* joints = (const uint2*)c->skin_joints.p;
    const float4* weights = (const float4*)c->skin_weights.p;
    float* vtx = (float*)c->up_vtx.p;
    auto rigid = batch_of<VertexTransformDev>([&](const VertexTransformDev& g) { fovpt_launch_transform_vertices_dev(st, g, rest, vtx); });
    auto skinned = batch_of<VertexSkin>([&](const VertexSkin& g) { fovpt_launch_skin_vertices(st, g, rest, joints, weights, vtx); });
    auto morphed = batch_of<VertexMorph>([&](const VertexMorph& g) { fovpt_launch_morph_vertices(st, g, rest, off, ent, vtx); });
    auto both = batch_of<VertexMorph>([&](const VertexMorph& g) { fovpt_launch_morph_skin_vertices(st, g, rest, off, ent, joints, weights, vtx); });
    for (const fovpt_ctx::RigBound& B : R.bound) {
        const uint32_t n = c->mesh_nv[B.mesh], first = c->mesh_vbase[B.mesh];
        if (B.is_rigid) rigid.add(n, [&](VertexTransformDev& g, int i) { g.m[i] = d.rigid + 12 * (size_t)B.rigid; g.first[i] = first; });
        else if (!B.morphed)
            skinned.add(n, [&](VertexSkin& g, int i) {
                g.pal[i] = d.skin_pal + 12 * (size_t)c->skins[B.mesh].pal_first; g.first[i] = first; g.skin[i] = c->skins[B.mesh].first;
            });
        else {
            auto fill = [&](VertexMorph& g, int i) {
                const fovpt_ctx::Morph& M = c->morphs[B.mesh];
                g.w[i] = d.morph_w + M.w_first; g.first[i] = first; g.off[i] = M.off_first;
                if (!B.skinned) return;
                g.pal[i] = d.skin_pal + 12 * (size_t)c->skins[B.mesh].pal_first; g.skin[i] = c->skins[B.mesh].first;
            };
            if (B.skinned) both.add(n, fill); else morphed.add(n, fill);
        }
    }
    rigid.flush(); skinned.flush(); morphed.flush(); both.flush();
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

// the rig goes (the caller has seen to it that nothing on the device still reads it)
void drop_rig(fovpt_ctx* c)
{
    c->rig.set = false;
    c->rig.num_clips = 0;
    c->rig.bound.clear();
    c->rig.in.release(); c->rig.out.release();
    c->rig.dev = RigDev{};
}

// How fovpt_set_skins, fovpt_set_morphs and fovpt_set_rig end once their plan is accepted.  The new device buffers (bytes[i] 0: none)
// are there before anything changes; `before` uploads what needs nothing of the context; then the wait for an update in flight,
// which reads the buffers about to go; the rig goes (its counts were checked against the skins and morphs about to change);
// `commit` moves the host state in and uploads from it; and the new buffers take the place of the old.
template <int N, class Before, class Commit>
int replace_buffers(fovpt_ctx* c, DevBuf* const (&live)[N], const size_t (&bytes)[N], Before before, Commit commit)
{
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf fresh[N];
    for (int i = 0; i < N; i++)
        if (bytes[i]) HIPCHK(c, fresh[i].reserve(bytes[i]));
    CHK(before(fresh));
    HIPCHK(c, hipStreamSynchronize(c->shadow_stream));
    drop_rig(c);
    CHK(commit(fresh));
    for (int i = 0; i < N; i++) live[i]->swap(fresh[i]);
    return FOVPT_OK;
}

}  // namespace

// The builder's thread is joined first (the slot's destructor would do it too late for the stream it works on)
fovpt_ctx::Rebuild::~Rebuild()
{
    (void)job.discard(free_rebuild_result);
    if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    if (ev_snapshot) (void)hipEventDestroy(ev_snapshot);
    if (rec) (void)hipHostFree(rec);
}

// What the calls of this file keep of a scene, dropped with it (fovpt_set_scene and the context's destructor; the device is
// idle): the device copies an update makes and the refit it may have left for the next job to wait for, fovpt_temporal_motion's
// tracking (switched on again by its next call), the rest positions and their bounds, the skins, the morph targets and the rig.
void drop_animation(fovpt_ctx* c)
{
    // a background rebuild of the scene that goes: joined and discarded; what adoptions retired; the snapshot's buffers
    end_background_rebuild(c);
    retire_idle(c);
    if (c->rb) { c->rb->flat.release(); c->rb->mesh_of.release(); std::vector<uint32_t>().swap(c->rb->in.h_mesh_of); }
    drop_rig(c);
    c->up_vtx.release(); c->up_vidx.release();
    c->engine.refit_pending = false;
    c->tm_tracking = c->tm_untracked = false;
    c->tm_mark.release(); c->vtx_prev.release();
    c->rest_vtx.release(); c->mesh_absmax.clear();
    c->skins.clear();
    c->skin_joints.release(); c->skin_weights.release(); c->skin_pal.release();
    c->morphs.clear();
    c->morph_off.release(); c->morph_ent.release(); c->morph_w.release();
}

extern "C" {

int fovpt_update_vertices(fovpt_ctx* c, const fovpt_vertex_update* up, int num_updates, int flags)
{
    const char* who = "fovpt_update_vertices";
    Listed L;
    CHK(L.open(c, who, num_updates, up, "updates", flags, FOVPT_UPDATE_DEVICE | FOVPT_UPDATE_REBUILD | FOVPT_UPDATE_REBUILD_ASYNC));
    const bool device = (flags & FOVPT_UPDATE_DEVICE) != 0;
    size_t floats = 0;
    for (int k = 0; k < num_updates; k++) {
        const fovpt_vertex_update& U = up[k];
        CHK(L.mesh(U.mesh));
        if (U.num_vertices != c->mesh_nv[U.mesh])
            return fail(c, FOVPT_E_INVALID, "%s: mesh %d has %u vertices, the update %u", who, U.mesh, c->mesh_nv[U.mesh], U.num_vertices);
        if (!U.vertex) return fail(c, FOVPT_E_INVALID, "%s: mesh %d has a null vertex pointer", who, U.mesh);
        if (!device)
            for (size_t i = 0; i < 3 * (size_t)U.num_vertices; i++)
                if (!std::isfinite(U.vertex[i])) return fail(c, FOVPT_E_INVALID, "%s: mesh %d vertex %zu is not finite", who, U.mesh, i / 3);
        floats += 3 * (size_t)U.num_vertices;
    }
    return update(L, flags, false, [&] { return device ? write_device(c, up, num_updates) : write_host(c, up, num_updates, floats); });
}

// The overflow rule keeps every intermediate value finite, so no device memory has to be read to know the coordinates are.
int fovpt_update_transforms(fovpt_ctx* c, const fovpt_mesh_transform* tf, int num, int flags)
{
    const char* who = "fovpt_update_transforms";
    Listed L;
    CHK(L.open(c, who, num, tf, "transforms", flags, FOVPT_UPDATE_REBUILD | FOVPT_UPDATE_REBUILD_ASYNC,
                "%s: flag bits %d (FOVPT_UPDATE_REBUILD and FOVPT_UPDATE_REBUILD_ASYNC are the only ones accepted)"));
    if (num > 0) ensure_absmax(c);
    for (int k = 0; k < num; k++) {
        const fovpt_mesh_transform& T = tf[k];
        CHK(L.mesh(T.mesh));
        AnimVerdict V;
        if (anim_check_transform(V, who, T.mesh, T.m, c->mesh_absmax[T.mesh])) return refused(c, V);
    }
    return update(L, flags, tf != nullptr, [&] { return write_transforms(c, tf, num); });
}

// The skins are kept on the host per mesh; every call lays the device copies out anew (plan_skins), so a mesh's places in
// skin_joints / skin_weights / skin_pal are fixed until the next call.
int fovpt_set_skins(fovpt_ctx* c, const fovpt_mesh_skin* skins, int num)
{
    const char* who = "fovpt_set_skins";
    Listed L;
    CHK(L.open(c, who, num, skins, "skins"));
    SkinPlan P;
    if (plan_skins(anim_scene(c), who, skins, num, P)) return refused(c, P);
    if (num == 0) return FOVPT_OK;
    DevBuf* const live[3] = {&c->skin_joints, &c->skin_weights, &c->skin_pal};
    const size_t bytes[3] = {P.joints_bytes, P.weights_bytes, P.pal_bytes};
    return replace_buffers(c, live, bytes, [](DevBuf*) { return FOVPT_OK; }, [&](DevBuf* fresh) {
        if (c->skins.empty()) c->skins.resize((size_t)L.nmesh);
        for (int k = 0; k < num; k++) {
            const fovpt_mesh_skin& K = skins[k];
            fovpt_ctx::Skin& D = c->skins[K.mesh];
            D.num_joints = K.num_joints; D.S = P.S[k];
            if (K.num_joints) { D.joints.assign(K.joints, K.joints + 4 * (size_t)K.num_vertices); D.weights.assign(K.weights, K.weights + 4 * (size_t)K.num_vertices); }
            else { std::vector<uint16_t>().swap(D.joints); std::vector<float>().swap(D.weights); }
        }
        for (int m = 0; m < L.nmesh; m++) {
            fovpt_ctx::Skin& D = c->skins[m];
            D.first = P.first[m]; D.pal_first = P.pal_first[m];
            if (!D.num_joints || !c->mesh_nv[m]) continue;
            HIPCHK(c, hipMemcpy((char*)fresh[0].p + 8 * (size_t)D.first, D.joints.data(), 8 * (size_t)c->mesh_nv[m], hipMemcpyHostToDevice));
            HIPCHK(c, hipMemcpy((char*)fresh[1].p + 16 * (size_t)D.first, D.weights.data(), 16 * (size_t)c->mesh_nv[m], hipMemcpyHostToDevice));
        }
        return FOVPT_OK;
    });
}

// For host palettes the overflow rules keep every intermediate value finite, as fovpt_update_transforms' does.
int fovpt_update_skinned(fovpt_ctx* c, const fovpt_skin_pose* poses, int num, int flags)
{
    const char* who = "fovpt_update_skinned";
    Listed L;
    CHK(L.open(c, who, num, poses, "poses", flags, FOVPT_UPDATE_DEVICE | FOVPT_UPDATE_REBUILD | FOVPT_UPDATE_REBUILD_ASYNC));
    const bool device = (flags & FOVPT_UPDATE_DEVICE) != 0;
    if (num > 0 && !device) ensure_absmax(c);
    size_t floats = 0;
    for (int k = 0; k < num; k++) {
        const fovpt_skin_pose& P = poses[k];
        CHK(L.mesh(P.mesh));
        if (c->skins.empty() || !c->skins[P.mesh].num_joints) return fail(c, FOVPT_E_INVALID, "%s: mesh %d has no skin", who, P.mesh);
        const fovpt_ctx::Skin& K = c->skins[P.mesh];
        if (P.num_joints != K.num_joints) return fail(c, FOVPT_E_INVALID, "%s: mesh %d: %u joints, its skin has %u", who, P.mesh, P.num_joints, K.num_joints);
        if (!P.matrices) return fail(c, FOVPT_E_INVALID, "%s: mesh %d: null matrices", who, P.mesh);
        floats += 12 * (size_t)P.num_joints;
        AnimVerdict V;
        if (!device && anim_check_palette(V, who, P.mesh, P.matrices, P.num_joints, K.S, c->mesh_absmax[P.mesh])) return refused(c, V);
    }
    return update(L, flags, poses != nullptr, [&] { return write_skinned(c, poses, num, device, floats); });
}

// The morph targets are kept on the host per mesh, transposed into a per-vertex list (plan_morphs; one launch does a whole pose: a
// pass per active target would need ordering between passes).  Every call lays the device copies out anew, so a mesh's places
// in morph_off / morph_ent / morph_w are fixed until the next call.
int fovpt_set_morphs(fovpt_ctx* c, const fovpt_mesh_morph* morphs, int num)
{
    const char* who = "fovpt_set_morphs";
    Listed L;
    CHK(L.open(c, who, num, morphs, "morphs"));
    MorphPlan P;
    if (plan_morphs(anim_scene(c), who, morphs, num, P)) return refused(c, P);
    if (num == 0) return FOVPT_OK;
    DevBuf* const live[3] = {&c->morph_off, &c->morph_ent, &c->morph_w};
    const size_t bytes[3] = {P.off_bytes, P.ent_bytes, P.w_bytes};
    return replace_buffers(c, live, bytes, [](DevBuf*) { return FOVPT_OK; }, [&](DevBuf* fresh) {
        if (c->morphs.empty()) c->morphs.resize((size_t)L.nmesh);
        for (int k = 0; k < num; k++) {
            fovpt_ctx::Morph& D = c->morphs[morphs[k].mesh];
            D.D = std::move(P.listed[k].D); D.off = std::move(P.listed[k].off); D.ent = std::move(P.listed[k].ent);
        }
        std::vector<uint32_t> abs_off;
        for (int m = 0; m < L.nmesh; m++) {
            fovpt_ctx::Morph& D = c->morphs[m];
            D.num_targets = P.num_targets[m]; D.off_first = P.off_first[m]; D.ent_first = P.ent_first[m]; D.w_first = P.w_first[m];
            if (!D.num_targets) continue;
            abs_off.resize(D.off.size());
            for (size_t i = 0; i < D.off.size(); i++) abs_off[i] = D.ent_first + D.off[i];
            HIPCHK(c, hipMemcpy((uint32_t*)fresh[0].p + D.off_first, abs_off.data(), 4 * abs_off.size(), hipMemcpyHostToDevice));
            if (!D.ent.empty()) HIPCHK(c, hipMemcpy((MorphEntry*)fresh[1].p + D.ent_first, D.ent.data(), 16 * D.ent.size(), hipMemcpyHostToDevice));
        }
        return FOVPT_OK;
    });
}

// For host data the overflow rules keep every intermediate value finite.
int fovpt_update_morphed(fovpt_ctx* c, const fovpt_morph_pose* poses, int num, int flags)
{
    const char* who = "fovpt_update_morphed";
    Listed L;
    CHK(L.open(c, who, num, poses, "poses", flags, FOVPT_UPDATE_DEVICE | FOVPT_UPDATE_REBUILD | FOVPT_UPDATE_REBUILD_ASYNC));
    const bool device = (flags & FOVPT_UPDATE_DEVICE) != 0;
    if (num > 0 && !device) ensure_absmax(c);
    size_t floats = 0;
    for (int k = 0; k < num; k++) {
        const fovpt_morph_pose& P = poses[k];
        CHK(L.mesh(P.mesh));
        if (P._reserved) return fail(c, FOVPT_E_INVALID, "%s: mesh %d: _reserved is %u", who, P.mesh, P._reserved);
        if (c->morphs.empty() || !c->morphs[P.mesh].num_targets) return fail(c, FOVPT_E_INVALID, "%s: mesh %d has no morph targets", who, P.mesh);
        const fovpt_ctx::Morph& M = c->morphs[P.mesh];
        if (P.num_targets != M.num_targets) return fail(c, FOVPT_E_INVALID, "%s: mesh %d: %u targets, the mesh has %u", who, P.mesh, P.num_targets, M.num_targets);
        if (!P.weights) return fail(c, FOVPT_E_INVALID, "%s: mesh %d: null weights", who, P.mesh);
        if ((P.matrices == nullptr) != (P.num_joints == 0))
            return fail(c, FOVPT_E_INVALID, "%s: mesh %d: %u joints with matrices at %p", who, P.mesh, P.num_joints, (const void*)P.matrices);
        const fovpt_ctx::Skin* K = nullptr;
        if (P.num_joints) {
            if (c->skins.empty() || !c->skins[P.mesh].num_joints) return fail(c, FOVPT_E_INVALID, "%s: mesh %d has no skin", who, P.mesh);
            K = &c->skins[P.mesh];
            if (P.num_joints != K->num_joints) return fail(c, FOVPT_E_INVALID, "%s: mesh %d: %u joints, its skin has %u", who, P.mesh, P.num_joints, K->num_joints);
        }
        floats += (size_t)P.num_targets + 12 * (size_t)P.num_joints;
        if (device) continue;
        AnimVerdict V;
        double B;      // the morphed positions' bound
        if (anim_check_weights(V, who, P.mesh, P.weights, P.num_targets, M.D.data(), c->mesh_absmax[P.mesh], &B)) return refused(c, V);
        if (K && anim_check_palette(V, who, P.mesh, P.matrices, P.num_joints, K->S, B)) return refused(c, V);
    }
    return update(L, flags, poses != nullptr, [&] { return write_morphed(c, poses, num, device, floats); });
}

// The rules and the layout are plan_rig's.  The device copy is uploaded whole before the previous rig goes.
int fovpt_set_rig(fovpt_ctx* c, const fovpt_rig_desc* rig)
{
    const char* who = "fovpt_set_rig";
    if (!c) return FOVPT_E_INVALID;
    if (!c->has_scene) return fail(c, FOVPT_E_NO_SCENE, "%s without a scene", who);
    if (!rig) {
        if (!c->rig.set) return FOVPT_OK;
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(c->shadow_stream));     // a fovpt_update_animated in flight reads the buffers about to go
        drop_rig(c);
        return FOVPT_OK;
    }
    RigPlan P;
    if (plan_rig(anim_scene(c), who, rig, P)) return refused(c, P);
    fovpt_ctx::Rig& R = c->rig;
    DevBuf* const live[2] = {&R.in, &R.out};
    const size_t bytes[2] = {P.blob.size() + 16, 4 * P.outs};
    return replace_buffers(c, live, bytes, [&](DevBuf* fresh) {
        HIPCHK(c, hipMemcpy(fresh[0].p, P.blob.data(), P.blob.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemset(fresh[1].p, 0, 4 * P.outs));
        return FOVPT_OK;
    }, [&](DevBuf* fresh) {
        R.bound.swap(P.bound);
        R.num_clips = P.num_clips;
        R.threads = P.threads;
        const char* in = (const char*)fresh[0].p;
        RigDev& D = R.dev;
        D.num_nodes = P.num_nodes; D.num_levels = P.num_levels; D.num_pal = (uint32_t)P.pal_node.size(); D.num_rigid = (uint32_t)P.rigid_node.size();
        D.num_wjobs = (uint32_t)P.wjobs.size();
        D.parent = (const int32_t*)(in + P.at[RIG_PARENT]); D.level = (const uint32_t*)(in + P.at[RIG_LEVEL]); D.rest = (const float*)(in + P.at[RIG_REST]);
        D.node_chan = (const int32_t*)(in + P.at[RIG_NODE_CHAN]); D.w_chan = (const int32_t*)(in + P.at[RIG_W_CHAN]); D.chan = (const RigChannel*)(in + P.at[RIG_CHAN]);
        D.times = (const float*)(in + P.at[RIG_TIMES]); D.values = (const float*)(in + P.at[RIG_VALUES]);
        D.pal_node = (const uint32_t*)(in + P.at[RIG_PAL_NODE]); D.pal_dst = (const uint32_t*)(in + P.at[RIG_PAL_DST]); D.inv_bind = (const float*)(in + P.at[RIG_INV_BIND]);
        D.rigid_node = (const uint32_t*)(in + P.at[RIG_RIGID_NODE]); D.wjobs = (const RigWeights*)(in + P.at[RIG_WJOBS]);
        D.world = (float*)fresh[1].p; D.rigid = D.world + 12 * (size_t)D.num_nodes; D.palette = D.rigid + 12 * (size_t)D.num_rigid;
        R.set = true;
        return FOVPT_OK;
    });
}

// The composed matrices are made on the device and not validated, as FOVPT_UPDATE_DEVICE pointers are not.
int fovpt_update_animated(fovpt_ctx* c, int clip, float time, int flags)
{
    const char* who = "fovpt_update_animated";
    Listed L;
    CHK(L.open(c, who, 0, nullptr, "clips", flags, FOVPT_UPDATE_REBUILD | FOVPT_UPDATE_REBUILD_ASYNC,
                "%s: flag bits %d (FOVPT_UPDATE_REBUILD and FOVPT_UPDATE_REBUILD_ASYNC are the only ones accepted)"));
    if (!c->rig.set) return fail(c, FOVPT_E_INVALID, "%s: no rig (fovpt_set_rig; fovpt_set_skins, fovpt_set_morphs and fovpt_set_scene drop it)", who);
    if (clip < 0 || (uint32_t)clip >= c->rig.num_clips) return fail(c, FOVPT_E_INVALID, "%s: clip %d of %u", who, clip, c->rig.num_clips);
    if (!std::isfinite(time)) return fail(c, FOVPT_E_INVALID, "%s: the time is not finite", who);
    for (const fovpt_ctx::RigBound& B : c->rig.bound) CHK(L.mesh(B.mesh));
    return update(L, flags, true, [&] { return write_animated(c, clip, time); });
}

// Polls, and with the flags waits for the builder's thread (never for the device) and adopts.  The text of a build that failed
// since the last call goes to the context here, on the caller's thread: the call itself succeeds.
int fovpt_rebuild_state(fovpt_ctx* c, int flags, fovpt_rebuild_info* out)
{
    const char* who = "fovpt_rebuild_state";
    if (!c) return FOVPT_E_INVALID;
    if (!out) return fail(c, FOVPT_E_INVALID, "%s: null out pointer", who);
    if (flags & ~(FOVPT_REBUILD_WAIT | FOVPT_REBUILD_ADOPT)) return fail(c, FOVPT_E_INVALID, "%s: unknown flag bits %d", who, flags);
    if (!c->has_scene) return fail(c, FOVPT_E_NO_SCENE, "%s without a scene", who);
    memset(out, 0, sizeof(*out));
    fovpt_ctx::Rebuild* R = c->rb.get();
    if (!R) return FOVPT_OK;                               // the context has never asked: idle, nothing counted
    HIPCHK(c, hipSetDevice(c->device));
    retire_poll(c);
    if (flags & FOVPT_REBUILD_WAIT) (void)R->job.wait();
    if (flags & FOVPT_REBUILD_ADOPT) CHK(adopt_ready(c));
    out->state = (int32_t)R->job.state();
    const RebuildJob::Counters& n = R->job.counters();
    out->last_error = R->job.last_error();
    out->requested = n.requested; out->started = n.started; out->adopted = n.adopted; out->failed = n.failed; out->discarded = n.discarded;
    out->snapshot_update = R->snapshot_update;
    const fovpt_ctx::RebuildDone* waiting = R->job.peek();
    out->ms_build = waiting ? (double)waiting->ms : R->ms_build;
    if (n.failed != R->failed_told) {
        R->failed_told = n.failed;
        (void)fail(c, R->job.last_error(), "background rebuild: %s", R->job.last_text().c_str());
    }
    return FOVPT_OK;
}

}  // extern "C"
