// api_animate.hip -- animated geometry over the C ABI (include/fovpt.h; kernels: refit.hip): fovpt_update_vertices,
// fovpt_update_transforms, fovpt_set_skins / fovpt_update_skinned, fovpt_set_morphs / fovpt_update_morphed.
//
// Every entry point validates all of its arguments first (all or nothing; Listed is the part they share).  An update is then
// three steps on fovpt_stream(), the stream every job's resolve, and so every job's last traversal launch, is ordered on:
// begin_update (what has to happen ahead of any new position), the source's own write_* (the new positions into up_vtx) and
// finish_update (the refit, with the event the next job waits for, or the rebuild).  A new source is a new write_*.
#include <cmath>
#include <cstring>

#include "fovpt_ctx.h"

#define CHK(x) do { const int rc_ = (x); if (rc_) return rc_; } while (0)

namespace {

// What the six entry points check first, in this order: open() the context, the scene, the count and the array (`what`: the
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
        seen.assign((size_t)nmesh, 0);
        return FOVPT_OK;
    }
    int check(int m)
    {
        if (m < 0 || m >= nmesh) return fail(c, FOVPT_E_INVALID, "%s: mesh %d of %d", who, m, nmesh);
        if (seen[m]) return fail(c, FOVPT_E_INVALID, "%s: mesh %d is listed twice", who, m);
        seen[m] = 1;
        return FOVPT_OK;
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

// The overflow rules of a host palette (fovpt_update_skinned, fovpt_update_morphed), which keep every intermediate value of the
// skinning expression finite: S the skin's largest weight sum, B a bound of the |coordinates| that go through the matrices.
// (Not fovpt_update_transforms' rule: one matrix is not blended, so that rule has no second part.)
int check_palette(fovpt_ctx* c, const char* who, int mesh, const float* matrices, uint32_t num_joints, double S, double B)
{
    for (size_t i = 0; i < 12 * (size_t)num_joints; i++)
        if (!std::isfinite(matrices[i])) return fail(c, FOVPT_E_INVALID, "%s: mesh %d joint %zu entry %zu is not finite", who, mesh, i / 12, i % 12);
    for (size_t r = 0; r < 3 * (size_t)num_joints; r++) {
        const float* row = matrices + 4 * r;
        const double bound = S * ((std::fabs((double)row[0]) + std::fabs((double)row[1]) + std::fabs((double)row[2])) * B + std::fabs((double)row[3]));
        if (bound > 0x1p127) return fail(c, FOVPT_E_INVALID, "%s: mesh %d joint %zu row %zu could overflow (bound %g > 2^127)", who, mesh, r / 3, r % 3, bound);
        // (the blended matrix is formed first: its entries are within S times the palette's, which the row's bound covers
        // for the fourth column and, for the others, only when B >= 1)
        const double entry = S * std::fmax(std::fmax(std::fabs((double)row[0]), std::fabs((double)row[1])), std::fabs((double)row[2]));
        if (entry > 0x1p127) return fail(c, FOVPT_E_INVALID, "%s: mesh %d joint %zu row %zu: a blended entry could overflow (%g > 2^127)", who, mesh, r / 3, r % 3, entry);
    }
    return FOVPT_OK;
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

// ---- the three steps of an update -----------------------------------------------------------------------------------------
// Ahead of the new positions of the listed meshes: a rebuild waits for the device; the scene's first update makes the device
// copies of what fovpt_set_scene kept; fovpt_temporal_motion's tracking copies the positions about to be overwritten; from_rest
// (the source reads the rest positions: its caller passed an array, if an empty one): the scene's first puts them on the device.
int begin_update(fovpt_ctx* c, const std::vector<int>& meshes, bool rebuild, bool from_rest)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (rebuild) CHK(sync_all(c));
    const hipStream_t st = c->shadow_stream;
    if (!c->up_vtx.p) {
        // the first update: the device copies of what fovpt_set_scene kept (ordered on the stream like everything below)
        if (!c->ev_scene) HIPCHK(c, hipEventCreateWithFlags(&c->ev_scene, hipEventDisableTiming));
        for (auto& S : c->up_stage)
            if (!S.ev) HIPCHK(c, hipEventCreateWithFlags(&S.ev, hipEventDisableTiming));
        HIPCHK(c, c->up_vidx.reserve(c->h_tri_vidx.size() * 4));
        HIPCHK(c, c->up_vtx.reserve(c->h_vtx.size() * 4));
        HIPCHK(c, hipMemcpyAsync(c->up_vidx.p, c->h_tri_vidx.data(), c->h_tri_vidx.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->up_vtx.p, c->h_vtx.data(), c->h_vtx.size() * 4, hipMemcpyHostToDevice, st));
    }
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
int finish_update(fovpt_ctx* c, bool rebuild)
{
    const hipStream_t st = c->shadow_stream;
    const float* vtx = (const float*)c->up_vtx.p;
    if (!rebuild) {
        fovpt_launch_refit(st, c->nodes, c->tris, c->bvh_levels, c->bvh_num_levels, (const uint3*)c->up_vidx.p, vtx);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->ev_scene, st));
        c->refit_pending = true;
        c->cost_updates++;
        fovpt_ctx::CostSlot* S = nullptr;
        return c->cost_watching ? enqueue_cost(c, st, c->cost_updates, &S) : FOVPT_OK;
    }
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

// What the four update calls do once everything is validated
template <class Write> int update(const Listed& L, bool rebuild, bool from_rest, Write write)
{
    CHK(check_updatable(L.c, L.who));
    if (L.meshes.empty() && !rebuild) return FOVPT_OK;
    CHK(begin_update(L.c, L.meshes, rebuild, from_rest));
    CHK(write());
    return finish_update(L.c, rebuild);
}

// ---- the five sources: validated entries to new positions in up_vtx -------------------------------------------------------
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

}  // namespace

// What the calls of this file keep of a scene, dropped with it (fovpt_set_scene and the context's destructor; the device is
// idle): the device copies an update makes and the refit it may have left for the next job to wait for, fovpt_temporal_motion's
// tracking (switched on again by its next call), the rest positions and their bounds, the skins and the morph targets.
void drop_animation(fovpt_ctx* c)
{
    c->up_vtx.release(); c->up_vidx.release();
    c->refit_pending = false;
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
    CHK(L.open(c, who, num_updates, up, "updates", flags, FOVPT_UPDATE_DEVICE | FOVPT_UPDATE_REBUILD));
    const bool device = (flags & FOVPT_UPDATE_DEVICE) != 0, rebuild = (flags & FOVPT_UPDATE_REBUILD) != 0;
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
    return update(L, rebuild, false, [&] { return device ? write_device(c, up, num_updates) : write_host(c, up, num_updates, floats); });
}

// The overflow rule keeps every intermediate value finite, so no device memory has to be read to know the coordinates are.
int fovpt_update_transforms(fovpt_ctx* c, const fovpt_mesh_transform* tf, int num, int flags)
{
    const char* who = "fovpt_update_transforms";
    Listed L;
    CHK(L.open(c, who, num, tf, "transforms", flags, FOVPT_UPDATE_REBUILD, "%s: flag bits %d (FOVPT_UPDATE_REBUILD is the only one accepted)"));
    if (num > 0) ensure_absmax(c);
    for (int k = 0; k < num; k++) {
        const fovpt_mesh_transform& T = tf[k];
        CHK(L.mesh(T.mesh));
        for (int i = 0; i < 12; i++)
            if (!std::isfinite(T.m[i])) return fail(c, FOVPT_E_INVALID, "%s: mesh %d matrix entry %d is not finite", who, T.mesh, i);
        for (int r = 0; r < 3; r++) {
            const float* row = T.m + 4 * r;
            const double bound = (std::fabs((double)row[0]) + std::fabs((double)row[1]) + std::fabs((double)row[2])) * c->mesh_absmax[T.mesh] + std::fabs((double)row[3]);
            if (bound > 0x1p127) return fail(c, FOVPT_E_INVALID, "%s: mesh %d row %d could overflow (bound %g > 2^127)", who, T.mesh, r, bound);
        }
    }
    return update(L, (flags & FOVPT_UPDATE_REBUILD) != 0, tf != nullptr, [&] { return write_transforms(c, tf, num); });
}

// The skins are kept on the host per mesh; every call lays the device copies out anew (the skinned meshes' vertices and joints
// in mesh order), so a mesh's places in skin_joints / skin_weights / skin_pal are fixed until the next call.
int fovpt_set_skins(fovpt_ctx* c, const fovpt_mesh_skin* skins, int num)
{
    const char* who = "fovpt_set_skins";
    Listed L;
    CHK(L.open(c, who, num, skins, "skins"));
    const int nmesh = L.nmesh;
    std::vector<double> sums((size_t)(num > 0 ? num : 0), 0.0);
    for (int k = 0; k < num; k++) {
        const fovpt_mesh_skin& K = skins[k];
        CHK(L.check(K.mesh));
        if (K._reserved) return fail(c, FOVPT_E_INVALID, "%s: mesh %d: _reserved is %u", who, K.mesh, K._reserved);
        if (K.num_vertices != c->mesh_nv[K.mesh])
            return fail(c, FOVPT_E_INVALID, "%s: mesh %d has %u vertices, not %u", who, K.mesh, c->mesh_nv[K.mesh], K.num_vertices);
        if (K.num_joints > FOVPT_SKIN_MAX_JOINTS) return fail(c, FOVPT_E_INVALID, "%s: mesh %d: %u joints (at most %d)", who, K.mesh, K.num_joints, FOVPT_SKIN_MAX_JOINTS);
        if (K.num_joints == 0) {
            if (K.joints || K.weights) return fail(c, FOVPT_E_INVALID, "%s: mesh %d: no joints, but a pointer (removing a skin takes two null pointers)", who, K.mesh);
            continue;
        }
        if (!K.joints || !K.weights) return fail(c, FOVPT_E_INVALID, "%s: mesh %d: null joints or weights", who, K.mesh);
        for (size_t i = 0; i < 4 * (size_t)K.num_vertices; i++) {
            if (K.joints[i] >= K.num_joints) return fail(c, FOVPT_E_INVALID, "%s: mesh %d vertex %zu: joint %u of %u", who, K.mesh, i / 4, (unsigned)K.joints[i], K.num_joints);
            if (!(K.weights[i] >= 0.0f && K.weights[i] <= 1.0f)) return fail(c, FOVPT_E_INVALID, "%s: mesh %d vertex %zu: weight %g is not in [0, 1]", who, K.mesh, i / 4, (double)K.weights[i]);
        }
        for (size_t i = 0; i < (size_t)K.num_vertices; i++) {
            const float* w = K.weights + 4 * i;
            sums[k] = std::fmax(sums[k], (((double)w[0] + (double)w[1]) + (double)w[2]) + (double)w[3]);
        }
    }
    if (num == 0) return FOVPT_OK;
    // the new layout, and its device buffers before anything changes
    std::vector<uint32_t> nj((size_t)nmesh, 0);
    for (int m = 0; m < nmesh; m++) nj[m] = c->skins.empty() ? 0 : c->skins[m].num_joints;
    for (int k = 0; k < num; k++) nj[skins[k].mesh] = skins[k].num_joints;
    size_t verts = 0, joints = 0;
    for (int m = 0; m < nmesh; m++)
        if (nj[m]) { verts += c->mesh_nv[m]; joints += nj[m]; }
    if (verts >= (1ull << 32)) return fail(c, FOVPT_E_INVALID, "%s: more than 2^32 - 1 skinned vertices", who);
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf d_joints, d_weights, d_pal;
    if (joints) {
        HIPCHK(c, d_joints.reserve(verts ? verts * 8 : 8));
        HIPCHK(c, d_weights.reserve(verts ? verts * 16 : 16));
        HIPCHK(c, d_pal.reserve(joints * 48));
    }
    HIPCHK(c, hipStreamSynchronize(c->shadow_stream));     // a fovpt_update_skinned in flight reads the buffers about to go
    if (c->skins.empty()) c->skins.resize((size_t)nmesh);
    for (int k = 0; k < num; k++) {
        const fovpt_mesh_skin& K = skins[k];
        fovpt_ctx::Skin& D = c->skins[K.mesh];
        D.num_joints = K.num_joints; D.S = sums[k];
        if (K.num_joints) { D.joints.assign(K.joints, K.joints + 4 * (size_t)K.num_vertices); D.weights.assign(K.weights, K.weights + 4 * (size_t)K.num_vertices); }
        else { std::vector<uint16_t>().swap(D.joints); std::vector<float>().swap(D.weights); }
    }
    uint32_t first = 0, pal_first = 0;
    for (int m = 0; m < nmesh; m++) {
        fovpt_ctx::Skin& D = c->skins[m];
        D.first = first; D.pal_first = pal_first;
        if (!D.num_joints) continue;
        if (c->mesh_nv[m]) {
            HIPCHK(c, hipMemcpy((char*)d_joints.p + 8 * (size_t)first, D.joints.data(), 8 * (size_t)c->mesh_nv[m], hipMemcpyHostToDevice));
            HIPCHK(c, hipMemcpy((char*)d_weights.p + 16 * (size_t)first, D.weights.data(), 16 * (size_t)c->mesh_nv[m], hipMemcpyHostToDevice));
        }
        first += c->mesh_nv[m]; pal_first += D.num_joints;
    }
    c->skin_joints.swap(d_joints); c->skin_weights.swap(d_weights); c->skin_pal.swap(d_pal);
    return FOVPT_OK;
}

// For host palettes the overflow rules keep every intermediate value finite, as fovpt_update_transforms' does.
int fovpt_update_skinned(fovpt_ctx* c, const fovpt_skin_pose* poses, int num, int flags)
{
    const char* who = "fovpt_update_skinned";
    Listed L;
    CHK(L.open(c, who, num, poses, "poses", flags, FOVPT_UPDATE_DEVICE | FOVPT_UPDATE_REBUILD));
    const bool device = (flags & FOVPT_UPDATE_DEVICE) != 0, rebuild = (flags & FOVPT_UPDATE_REBUILD) != 0;
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
        if (!device) CHK(check_palette(c, who, P.mesh, P.matrices, P.num_joints, K.S, c->mesh_absmax[P.mesh]));
    }
    return update(L, rebuild, poses != nullptr, [&] { return write_skinned(c, poses, num, device, floats); });
}

// The morph targets are kept on the host per mesh, transposed into a per-vertex list of {delta, target} records sorted by
// target (what the kernel walks: the order of the definition is the order in memory, and one launch does a whole pose; a pass per
// active target would need ordering between passes).  Every call lays the device copies out anew (the morphed meshes' offsets,
// entries and weights in mesh order), so a mesh's places in morph_off / morph_ent / morph_w are fixed until the next call.
int fovpt_set_morphs(fovpt_ctx* c, const fovpt_mesh_morph* morphs, int num)
{
    const char* who = "fovpt_set_morphs";
    Listed L;
    CHK(L.open(c, who, num, morphs, "morphs"));
    const int nmesh = L.nmesh;
    std::vector<size_t> entries((size_t)(num > 0 ? num : 0), 0);
    for (int k = 0; k < num; k++) {
        const fovpt_mesh_morph& K = morphs[k];
        CHK(L.check(K.mesh));
        if (K._reserved) return fail(c, FOVPT_E_INVALID, "%s: mesh %d: _reserved is %u", who, K.mesh, K._reserved);
        const uint32_t nv = c->mesh_nv[K.mesh];
        if (K.num_vertices != nv) return fail(c, FOVPT_E_INVALID, "%s: mesh %d has %u vertices, not %u", who, K.mesh, nv, K.num_vertices);
        if (K.num_targets > FOVPT_MORPH_MAX_TARGETS) return fail(c, FOVPT_E_INVALID, "%s: mesh %d: %u targets (at most %d)", who, K.mesh, K.num_targets, FOVPT_MORPH_MAX_TARGETS);
        if (K.num_targets == 0) {
            if (K.targets) return fail(c, FOVPT_E_INVALID, "%s: mesh %d: no targets, but a pointer (removing morphs takes a null pointer)", who, K.mesh);
            continue;
        }
        if (!K.targets) return fail(c, FOVPT_E_INVALID, "%s: mesh %d: null targets", who, K.mesh);
        for (uint32_t t = 0; t < K.num_targets; t++) {
            const fovpt_morph_target& T = K.targets[t];
            if (T._reserved) return fail(c, FOVPT_E_INVALID, "%s: mesh %d target %u: _reserved is %u", who, K.mesh, t, T._reserved);
            if (T.count > nv) return fail(c, FOVPT_E_INVALID, "%s: mesh %d target %u: %u entries for %u vertices", who, K.mesh, t, T.count, nv);
            if (!T.index && T.count != 0 && T.count != nv)
                return fail(c, FOVPT_E_INVALID, "%s: mesh %d target %u: no indices, but %u entries for %u vertices", who, K.mesh, t, T.count, nv);
            if (!T.delta && T.count) return fail(c, FOVPT_E_INVALID, "%s: mesh %d target %u: null delta", who, K.mesh, t);
            entries[k] += T.count;
        }
    }
    if (num == 0) return FOVPT_OK;
    // the new layout (its size is known from the counts alone: checked before the entries themselves are read)
    std::vector<uint32_t> nt((size_t)nmesh, 0);
    std::vector<size_t> ne((size_t)nmesh, 0);
    for (int m = 0; m < nmesh && !c->morphs.empty(); m++) { nt[m] = c->morphs[m].num_targets; ne[m] = c->morphs[m].ent.size(); }
    for (int k = 0; k < num; k++) { nt[morphs[k].mesh] = morphs[k].num_targets; ne[morphs[k].mesh] = entries[k]; }
    size_t offs = 0, ents = 0, targets = 0;
    for (int m = 0; m < nmesh; m++)
        if (nt[m]) { offs += (size_t)c->mesh_nv[m] + 1; ents += ne[m]; targets += nt[m]; }
    if (ents >= (1ull << 32) || offs >= (1ull << 32)) return fail(c, FOVPT_E_INVALID, "%s: more than 2^32 - 1 entries (%zu) or offsets (%zu)", who, ents, offs);
    for (int k = 0; k < num; k++) {
        const fovpt_mesh_morph& K = morphs[k];
        for (uint32_t t = 0; t < K.num_targets; t++) {
            const fovpt_morph_target& T = K.targets[t];
            for (uint32_t i = 0; T.index && i < T.count; i++) {
                if (T.index[i] >= K.num_vertices) return fail(c, FOVPT_E_INVALID, "%s: mesh %d target %u entry %u: vertex %u of %u", who, K.mesh, t, i, T.index[i], K.num_vertices);
                if (i && T.index[i] <= T.index[i - 1]) return fail(c, FOVPT_E_INVALID, "%s: mesh %d target %u entry %u: indices are not strictly ascending", who, K.mesh, t, i);
            }
            for (size_t i = 0; i < 3 * (size_t)T.count; i++)
                if (!std::isfinite(T.delta[i])) return fail(c, FOVPT_E_INVALID, "%s: mesh %d target %u entry %zu: a delta is not finite", who, K.mesh, t, i / 3);
        }
    }
    // the named meshes' targets, transposed: a count per vertex, its running sum, then the targets in ascending order
    std::vector<fovpt_ctx::Morph> fresh((size_t)num);
    for (int k = 0; k < num; k++) {
        const fovpt_mesh_morph& K = morphs[k];
        fovpt_ctx::Morph& D = fresh[k];
        D.num_targets = K.num_targets;
        if (!K.num_targets) continue;
        const uint32_t nv = K.num_vertices;
        D.D.assign(K.num_targets, 0.0);
        D.off.assign((size_t)nv + 1, 0);
        for (uint32_t t = 0; t < K.num_targets; t++)
            for (uint32_t i = 0; i < K.targets[t].count; i++) D.off[(K.targets[t].index ? K.targets[t].index[i] : i) + 1]++;
        for (uint32_t i = 0; i < nv; i++) D.off[i + 1] += D.off[i];
        D.ent.resize(entries[k]);
        std::vector<uint32_t> fill(D.off.begin(), D.off.end() - 1);
        for (uint32_t t = 0; t < K.num_targets; t++) {
            const fovpt_morph_target& T = K.targets[t];
            for (uint32_t i = 0; i < T.count; i++) {
                const float* d = T.delta + 3 * (size_t)i;
                D.ent[fill[T.index ? T.index[i] : i]++] = MorphEntry{d[0], d[1], d[2], t};
                D.D[t] = std::fmax(D.D[t], std::fmax(std::fabs((double)d[0]), std::fmax(std::fabs((double)d[1]), std::fabs((double)d[2]))));
            }
        }
    }
    // the device buffers before anything changes
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf d_off, d_ent, d_w;
    if (targets) {
        HIPCHK(c, d_off.reserve(offs * 4));
        HIPCHK(c, d_ent.reserve(ents ? ents * 16 : 16));
        HIPCHK(c, d_w.reserve(targets * 4));
    }
    HIPCHK(c, hipStreamSynchronize(c->shadow_stream));     // a fovpt_update_morphed in flight reads the buffers about to go
    if (c->morphs.empty()) c->morphs.resize((size_t)nmesh);
    for (int k = 0; k < num; k++) c->morphs[morphs[k].mesh] = std::move(fresh[k]);
    uint32_t off_first = 0, ent_first = 0, w_first = 0;
    std::vector<uint32_t> abs_off;
    for (int m = 0; m < nmesh; m++) {
        fovpt_ctx::Morph& D = c->morphs[m];
        D.off_first = off_first; D.ent_first = ent_first; D.w_first = w_first;
        if (!D.num_targets) continue;
        abs_off.resize(D.off.size());
        for (size_t i = 0; i < D.off.size(); i++) abs_off[i] = ent_first + D.off[i];
        HIPCHK(c, hipMemcpy((uint32_t*)d_off.p + off_first, abs_off.data(), 4 * abs_off.size(), hipMemcpyHostToDevice));
        if (!D.ent.empty()) HIPCHK(c, hipMemcpy((MorphEntry*)d_ent.p + ent_first, D.ent.data(), 16 * D.ent.size(), hipMemcpyHostToDevice));
        off_first += (uint32_t)D.off.size(); ent_first += (uint32_t)D.ent.size(); w_first += D.num_targets;
    }
    c->morph_off.swap(d_off); c->morph_ent.swap(d_ent); c->morph_w.swap(d_w);
    return FOVPT_OK;
}

// For host data the overflow rules keep every intermediate value finite.
int fovpt_update_morphed(fovpt_ctx* c, const fovpt_morph_pose* poses, int num, int flags)
{
    const char* who = "fovpt_update_morphed";
    Listed L;
    CHK(L.open(c, who, num, poses, "poses", flags, FOVPT_UPDATE_DEVICE | FOVPT_UPDATE_REBUILD));
    const bool device = (flags & FOVPT_UPDATE_DEVICE) != 0, rebuild = (flags & FOVPT_UPDATE_REBUILD) != 0;
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
        double B = c->mesh_absmax[P.mesh];      // the morphed positions' bound
        for (uint32_t t = 0; t < P.num_targets; t++) {
            if (!std::isfinite(P.weights[t])) return fail(c, FOVPT_E_INVALID, "%s: mesh %d: weight %u is not finite", who, P.mesh, t);
            B += std::fabs((double)P.weights[t]) * M.D[t];
        }
        if (B > 0x1p127) return fail(c, FOVPT_E_INVALID, "%s: mesh %d could overflow (bound %g > 2^127)", who, P.mesh, B);
        if (K) CHK(check_palette(c, who, P.mesh, P.matrices, P.num_joints, K->S, B));
    }
    return update(L, rebuild, poses != nullptr, [&] { return write_morphed(c, poses, num, device, floats); });
}

}  // extern "C"
