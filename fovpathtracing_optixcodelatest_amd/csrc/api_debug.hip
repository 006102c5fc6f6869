// api_debug.hip -- the test hooks of the C ABI (include/fovpt.h, fovpt_debug_*): the production kernels and the device functions of
// a shaded hit on inputs a test lays out, launched as run_job (fovpt_api.hip) launches them.  No kernels: the device side is
// shade_debug.hip and the production kernel files.  A hook checks everything before it allocates, enqueues or writes anything.
#include <cstddef>
#include <cstring>

#include "fovpt_ctx.h"

namespace {

// Begin and end of a hook's device work: the context's device with nothing in flight ...
int debug_begin(fovpt_ctx* c)
{
    HIPCHK(c, hipSetDevice(c->device));
    return sync_all(c);
}
// ... and what the launches left as an error, then idle again
int debug_end(fovpt_ctx* c)
{
    HIPCHK(c, hipGetLastError());
    return sync_all(c);
}

// A host array into a buffer made for it, and the first n bytes of a buffer out (dst null: not asked for)
hipError_t upload(DevBuf& b, const void* src, size_t n)
{
    const hipError_t e = b.reserve(n);
    return e != hipSuccess ? e : hipMemcpy(b.p, src, n, hipMemcpyHostToDevice);
}
hipError_t download(void* dst, const DevBuf& b, size_t n) { return dst ? hipMemcpy(dst, b.p, n, hipMemcpyDeviceToHost) : hipSuccess; }

// An idle state set for a hook, as a job of `slots` sample slots and `launches` launch records sizes it, and its shard capacity
int debug_state(fovpt_ctx* c, size_t slots, size_t launches, StateSet*& S, uint32_t& cap)
{
    CHK(debug_begin(c));
    S = &c->engine.set[(c->engine.rot.last_set + 1u) % 2u];         // (the device is idle: any set will do)
    cap = shard_capacity(slots);
    return ensure_state(c, *S, slots, launches, c->stream);
}

// The frame a fovpt_launch (render = 0: a width x height grid; with row1 > 0 the chunk [row0, row1) of it, as run_passes hands a
// chunk to run_job) or a fovpt_render (render = 1) of these parameters would run -- frame_dev() is shared with run_job -- and its
// pass table for the caller `who`, which needs it to lay its arrays out.  A frame that would run as several jobs is refused.
int debug_frame(fovpt_ctx* c, const fovpt_launch_params* lp, int render, uint32_t width, uint32_t height, uint32_t row0, uint32_t row1,
                const char* who, FrameDev& fd, uint64_t& slots, uint64_t& launches, fovpt_debug_pass* passes_out, int* npass_out)
{
    PassDev P[FOVPT_MAX_PASSES];
    int npass = 1;
    if (render) { fovpt_launch_params L = *lp; npass = frame_passes(c->cfg, L, P); }
    else P[0] = pass_from_lp(lp, width, height);
    const bool chunk = row1 > 0u;
    uint64_t over = 0;
    CHK(job_passes(c, P, npass, 0u, row0, row1, P, &over));                                    // as run_passes hands a frame, or a chunk of a launch, to run_job
    if (over) return fail(c, FOVPT_E_INVALID, "%s: %llu sample slots would run as several jobs", who, (unsigned long long)over);
    CHK(frame_dev(c, lp, P, npass, chunk ? 1 : 0, render ? 1 : 0, nullptr, fd, slots, launches));
    *npass_out = npass;
    for (int p = 0; p < npass; p++) {
        const PassDev& D = fd.pass[p];
        passes_out[p].gw = D.gw; passes_out[p].rows = D.row1 - D.row0; passes_out[p].spp = D.spp;
        passes_out[p].slot_base = D.slot_base; passes_out[p].launch_base = D.launch_base;
    }
    return FOVPT_OK;
}

// The queue counters of a state set: the words in front of the statistics, shard s's word w at s * FOVPT_SHARD_STRIDE + w
const size_t cnt_bytes = offsetof(Counters, stat_radiance), cnt_words = cnt_bytes / 4;

// A host image onto a set's queue counters ...
hipError_t put_counters(StateSet& S, const std::vector<uint32_t>& cw, hipStream_t st) { return hipMemcpyAsync(S.counters.p, cw.data(), cnt_bytes, hipMemcpyHostToDevice, st); }
// ... and what everything enqueued on st left of them, with the set as a job expects to find it (resolve zeroes the queue
// counters at the end of every job)
int take_counters(fovpt_ctx* c, StateSet& S, std::vector<uint32_t>& cw, hipStream_t st)
{
    cw.resize(cnt_words);
    HIPCHK(c, hipMemcpyAsync(cw.data(), S.counters.p, cnt_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipMemset(S.counters.p, 0, cnt_bytes));
    return FOVPT_OK;
}

// The counter words that are not as they were, the words w0 and w1 of every shard aside (-1: none)
uint32_t counters_changed(const std::vector<uint32_t>& now, const std::vector<uint32_t>& was, int w0, int w1)
{
    uint32_t n = 0;
    for (size_t i = 0; i < cnt_words; i++) {
        const int w = (int)(i % FOVPT_SHARD_STRIDE);
        if (w != w0 && w != w1 && now[i] != was[i]) n++;
    }
    return n;
}

// The occupied entries of k arrays a[0 .. k) of qn 16-byte entries that held the byte `fill`: any word of the entry differs from
// the fill in any array.  Returns how many; the first `limit` in ascending physical order are handed out, entry e as place2 =
// (e / cap, e % cap) -- the shard and the index in it -- and its record of every array in rec4[0 .. k).
uint32_t occupied_entries(int k, const std::vector<uint32_t>* a, size_t qn, int fill, uint32_t cap, uint64_t limit, uint32_t* place2, float* const* rec4)
{
    const uint32_t fw = 0x01010101u * (uint32_t)fill;
    uint32_t n = 0;
    for (size_t e = 0; e < qn; e++) {
        bool occupied = false;
        for (int j = 0; j < k && !occupied; j++) occupied = a[j][4 * e] != fw || a[j][4 * e + 1] != fw || a[j][4 * e + 2] != fw || a[j][4 * e + 3] != fw;
        if (!occupied) continue;
        if ((uint64_t)n < limit) {
            place2[2 * (size_t)n] = (uint32_t)(e / cap); place2[2 * (size_t)n + 1] = (uint32_t)(e % cap);
            for (int j = 0; j < k; j++) memcpy(rec4[j] + 4 * (size_t)n, &a[j][4 * e], 16);
        }
        n++;
    }
    return n;
}

// test hooks: the device functions of a shaded hit on chosen inputs (shade_debug.hip), so that ProbeSample, ProbeEval, the
// Disney BSDF and tex2D can be compared with the oracle input by input, not only through frames.  The probe entry points take
// the caller's fovpt_probe the way a launch does and search it the way a launch would (probe_path).
int debug_probe_args(fovpt_ctx* c, const fovpt_probe* probe, int flags, int n, const void* in, const char* who)
{
    if (!c || !probe || n < 0 || (flags & ~FOVPT_DEBUG_PROBE_PLAIN) || (n && !in)) return FOVPT_E_INVALID;
    if (!probe_complete(*probe)) return fail(c, FOVPT_E_NO_PROBE, "%s with an incomplete probe", who);
    return FOVPT_OK;
}
ProbePath debug_probe_path(const fovpt_ctx* c, const fovpt_probe& probe, int flags, int* path_out)
{
    ProbePath pp = probe_path(c, probe);
    if (flags & FOVPT_DEBUG_PROBE_PLAIN) { pp.guide_x = pp.guide_y = nullptr; pp.rec = nullptr; pp.row_mul = 1; }
    if (path_out) *path_out = (pp.guide_x ? FOVPT_PROBE_PATH_GUIDED : 0) | (pp.rec ? FOVPT_PROBE_PATH_RECORDS : 0) | (pp.row_mul == 0 ? FOVPT_PROBE_PATH_ONE_ROW : 0);
    return pp;
}

static_assert(FOVPT_DEBUG_TRACE_ITERS == FOVPT_MAX_ITERS, "the iterations a traversal hook may name are the counter words there are");

// One of the two ray sets of a traversal hook (the selected chain's, the other chain's) and where its rays lie: ray i of the
// set is entry i - (the rays of the shards before) of the shard the counts put it in, in either queue
struct TraceRays {
    size_t n;
    const float *o3, *d3;
    const uint32_t *slot, *target;
    const float *vis4, *occ4;
    const uint32_t *q_count, *sq_count;
};

// What shard s of the six queue arrays holds for a traversal hook -- a[0 .. 6) = the radiance queue's o, d and the shadow queue's
// o, d, vis, occ, `cap` entries each: the rays the counts put there, then the idle ray
void trace_shard_image(const TraceRays* sets, int nsets, uint32_t s, uint32_t cap, const float* idle_o4, std::vector<float>* a)
{
    const float idle_d4[4] = {0.f, 1.f, 0.f, 0.f}, idle_vis4[4] = {3.f, 5.f, 7.f, 9.f}, idle_occ4[4] = {4.f, 6.f, 8.f, 10.f};
    const float* const idle[6] = {idle_o4, idle_d4, idle_o4, idle_d4, idle_vis4, idle_occ4};       // (a shadow record's d.w: cell 0, as bits)
    for (int k = 0; k < 6; k++) {
        a[k].resize((size_t)cap * 4);
        for (size_t e = 0; e < cap; e++) memcpy(&a[k][4 * e], idle[k], 16);
    }
    for (int t = 0; t < nsets; t++) {
        const TraceRays& R = sets[t];
        for (int shadow = 0; shadow < 2; shadow++) {
            const uint32_t* count = shadow ? R.sq_count : R.q_count;
            size_t i = 0;
            for (uint32_t k = 0; k < s; k++) i += count[k];
            for (uint32_t e = 0; e < count[s]; e++, i++) {
                float* o = &a[shadow ? 2 : 0][4 * (size_t)e];
                float* d = &a[shadow ? 3 : 1][4 * (size_t)e];
                for (int k = 0; k < 3; k++) { o[k] = R.o3[3 * i + k]; d[k] = R.d3[3 * i + k]; }
                memcpy(&o[3], &R.slot[i], 4);                            // origin.w = sample slot
                d[3] = 0.f;
                if (shadow) {
                    memcpy(&d[3], &R.target[i], 4);                      // shadow record: direction.w = target cell of the slot
                    memcpy(&a[4][4 * (size_t)e], &R.vis4[4 * i], 16);
                    memcpy(&a[5][4 * (size_t)e], &R.occ4[4 * i], 16);
                }
            }
        }
    }
}

// The shared step of fovpt_debug_trace and fovpt_debug_trace_queued (include/fovpt.h has the contract)
int trace_queued(fovpt_ctx* c, const fovpt_debug_trace_launch* in, fovpt_debug_trace_result* out, const char* who)
{
    if (!c || !in || !out || in->n < 0 || in->n_other < 0) return FOVPT_E_INVALID;
    if (in->n && (!in->origins3 || !in->dirs3 || !in->slot || !in->target || !in->vis4 || !in->occ4)) return FOVPT_E_INVALID;
    if (in->n_other && (!in->other_origins3 || !in->other_dirs3 || !in->other_slot || !in->other_target || !in->other_vis4 || !in->other_occ4)) return FOVPT_E_INVALID;
    if (!c->has_scene) return fail(c, FOVPT_E_NO_SCENE, "%s without a scene", who);
    if (c->cfg.max_depth < 1 || c->cfg.max_depth > 32) return fail(c, FOVPT_E_INVALID, "max_depth out of range");
    const uint32_t sel = in->sel;
    if (sel > 2u || ((in->n_other || in->both) && sel == 0u)) return fail(c, FOVPT_E_INVALID, "%s: sel %u with %d rays of another chain", who, sel, in->n_other);
    if (in->it_closest < 0 || in->it_closest >= FOVPT_MAX_ITERS || in->it_shadow < 0 || in->it_shadow >= FOVPT_MAX_ITERS)
        return fail(c, FOVPT_E_INVALID, "%s: iterations %d and %d", who, in->it_closest, in->it_shadow);
    if (in->grid_closest < 0 || in->grid_closest > (1 << 20) || in->grid_shadow < 0 || in->grid_shadow > (1 << 20))
        return fail(c, FOVPT_E_INVALID, "%s: grids %d and %d", who, in->grid_closest, in->grid_shadow);
    const size_t n = (size_t)in->n, m = (size_t)in->n_other, N = n + m, D = (size_t)c->cfg.max_depth;
    const size_t slots = in->slots ? (size_t)in->slots : (n ? n : 1u) * FOVPT_SHARDS;
    const uint32_t cap = shard_capacity(slots);
    const TraceRays sets[2] = {{n, in->origins3, in->dirs3, in->slot, in->target, in->vis4, in->occ4, in->q_count, in->sq_count},
                               {m, in->other_origins3, in->other_dirs3, in->other_slot, in->other_target, in->other_vis4, in->other_occ4,
                                in->other_q_count, in->other_sq_count}};
    for (int t = 0; t < 2; t++) {
        const TraceRays& R = sets[t];
        uint64_t total[2] = {0, 0};
        for (uint32_t s = 0; s < FOVPT_SHARDS; s++) {
            const bool selected = sel == 0u || (sel == 1u) == (s < 4u), mine = t == 0 ? selected : !selected;
            if ((R.q_count[s] || R.sq_count[s]) && !mine) return fail(c, FOVPT_E_INVALID, "%s: rays in shard %u outside the selection %u", who, s, t == 0 ? sel : 3u - sel);
            if (R.q_count[s] > cap || R.sq_count[s] > cap) return fail(c, FOVPT_E_INVALID, "%s: shard %u holds more than its capacity %u", who, s, cap);
            total[0] += R.q_count[s]; total[1] += R.sq_count[s];
        }
        if (total[0] != R.n || total[1] != R.n)
            return fail(c, FOVPT_E_INVALID, "%s: the shards hold %llu and %llu rays, n = %zu", who, (unsigned long long)total[0], (unsigned long long)total[1], R.n);
        std::vector<uint8_t> seen(R.n, 0);
        const size_t first = t == 0 ? 0 : n;
        for (size_t i = 0; i < R.n; i++) {
            const size_t k = (size_t)R.slot[i] - first;                  // (below `first`: wraps to a large number)
            if (R.slot[i] < first || k >= R.n || seen[k]) return fail(c, FOVPT_E_INVALID, "%s: the slots are no permutation (ray %zu names slot %u)", who, i, R.slot[i]);
            seen[k] = 1;
            if (R.target[i] != FOVPT_DEBUG_TRACE_ALPHA && R.target[i] >= D) return fail(c, FOVPT_E_INVALID, "%s: ray %zu names cell %u of %zu", who, i, R.target[i], D);
        }
    }
    for (uint32_t s = 0; s < FOVPT_SHARDS; s++)
        if (in->decoy[s] > cap) return fail(c, FOVPT_E_INVALID, "%s: a decoy count above the capacity %u", who, cap);
    if (!out->cells4 || !out->alpha4 || (N && (!out->hit_place2 || !out->hit4 || !out->hit_prim))) return FOVPT_E_INVALID;
    // the state: the queues of a job of `slots` sample slots, the cells of all N + 1
    StateSet* set = nullptr; uint32_t cap_state = 0;
    CHK(debug_state(c, slots > N + 1 ? slots : N + 1, 1, set, cap_state));
    StateSet& S = *set;
    hipStream_t st = c->stream;
    const size_t v = 16, qn = (size_t)cap * FOVPT_SHARDS;
    const int fill = FOVPT_DEBUG_SHADE_FILL;
    HIPCHK(c, hipMemsetAsync(S.s_hit.p, fill, qn * v, st));
    HIPCHK(c, hipMemsetAsync(S.s_rad.p, fill, (N + 1) * v * D, st));
    HIPCHK(c, hipMemsetAsync(S.s_alpha.p, fill, (N + 1) * v, st));
    // the idle ray: from the middle of the scene's vertices, along +y, for the trap slot N
    float idle_o4[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < 3 && c->h_vtx.size() >= 3; k++) {
        float lo = c->h_vtx[k], hi = lo;
        for (size_t i = k; i < c->h_vtx.size(); i += 3) { lo = c->h_vtx[i] < lo ? c->h_vtx[i] : lo; hi = c->h_vtx[i] > hi ? c->h_vtx[i] : hi; }
        idle_o4[k] = 0.5f * lo + 0.5f * hi;
    }
    const uint32_t trap = (uint32_t)N;
    memcpy(&idle_o4[3], &trap, 4);
    const DevBuf* const qbuf[6] = {&S.q_o[0], &S.q_d[0], &S.sq_o[0], &S.sq_d[0], &S.sq_vis[0], &S.sq_occ[0]};
    std::vector<float> image[6];
    for (uint32_t s = 0; s < FOVPT_SHARDS; s++) {
        trace_shard_image(sets, m ? 2 : 1, s, cap, idle_o4, image);
        for (int k = 0; k < 6; k++) HIPCHK(c, hipMemcpyAsync((char*)qbuf[k]->p + (size_t)s * cap * v, image[k].data(), (size_t)cap * v, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));                             // (the image is reused for the next shard)
    }
    // the counter words: the counts where the launches read them, the decoys in every word a neighbouring iteration would use
    const int w_q = FOVPT_CNT_Q(in->it_closest), w_sq = FOVPT_CNT_SQ(in->it_shadow);
    const int near[6] = {FOVPT_CNT_Q(in->it_closest - 1), FOVPT_CNT_Q(in->it_closest + 1), FOVPT_CNT_Q(in->it_shadow),
                         FOVPT_CNT_SQ(in->it_shadow - 1), FOVPT_CNT_SQ(in->it_shadow + 1), FOVPT_CNT_SQ(in->it_closest)};
    std::vector<uint32_t> was(cnt_words, 0u), cw;
    for (uint32_t s = 0; s < FOVPT_SHARDS; s++) {
        uint32_t* w = &was[(size_t)s * FOVPT_SHARD_STRIDE];
        for (int k = 0; k < 6; k++) {
            const bool radiance = k < 3;                                 // (it - 1 of iteration 0 names no word of its queue)
            const int lo = radiance ? FOVPT_CNT_Q(0) : FOVPT_CNT_SQ(0), hi = lo + FOVPT_MAX_ITERS;
            if (near[k] >= lo && near[k] <= hi) w[near[k]] = in->decoy[s];
        }
        w[w_q] = in->q_count[s] + in->other_q_count[s];
        w[w_sq] = in->sq_count[s] + in->other_sq_count[s];
    }
    HIPCHK(c, put_counters(S, was, st));
    Counters* cnt = (Counters*)S.counters.p;
    unsigned long long stat0[3], stat1[3];
    HIPCHK(c, hipMemcpyAsync(stat0, &cnt->stat_radiance, sizeof(stat0), hipMemcpyDeviceToHost, st));
    // (under write_guides the path state carries the set's guide buffers, which ensure_state has made: k_traverse never reads them)
    const PathState ps = path_state(c, S);
    const RayQueue q = ray_queue(S, 0);
    const ShadowQueue sq = shadow_queue(S, 0);
    const SceneView sc = scene_view(c);
    const int div = sel ? 2 : 1;                                         // a chain's launches get half the grids (run_job)
    const int g_trace = in->grid_closest ? in->grid_closest : c->engine.grid_trace / div, g_shadow = in->grid_shadow ? in->grid_shadow : c->engine.grid_shadow / div;
    for (int pass = 0; pass < (in->both ? 2 : 1); pass++) {
        const uint32_t sel_now = pass == 0 ? sel : 3u - sel;
        fovpt_launch_traverse(st, sc, ps, q, sq, cap, cnt, in->it_closest, -1, g_trace, nullptr, sel_now);    // closest hit, as run_job launches it
        fovpt_launch_traverse(st, sc, ps, q, sq, cap, cnt, -1, in->it_shadow, g_shadow, nullptr, sel_now);    // occlusion, as run_job launches it
    }
    HIPCHK(c, hipGetLastError());
    std::vector<uint32_t> hit(qn * 4);
    HIPCHK(c, hipMemcpyAsync(hit.data(), S.s_hit.p, qn * v, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(out->cells4, S.s_rad.p, (N + 1) * v * D, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(out->alpha4, S.s_alpha.p, (N + 1) * v, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(stat1, &cnt->stat_radiance, sizeof(stat1), hipMemcpyDeviceToHost, st));
    CHK(take_counters(c, S, cw, st));
    out->cap = cap;
    out->stat_radiance = stat1[0] - stat0[0]; out->stat_shadow = stat1[1] - stat0[1]; out->stat_paths = stat1[2] - stat0[2];
    out->counters_changed = counters_changed(cw, was, -1, -1);
    // the product build never writes a queue
    out->queues_unchanged = 1u;
    std::vector<float> back((size_t)cap * 4);
    for (uint32_t s = 0; s < FOVPT_SHARDS; s++) {
        trace_shard_image(sets, m ? 2 : 1, s, cap, idle_o4, image);
        for (int k = 0; k < 6; k++) {
            HIPCHK(c, hipMemcpy(back.data(), (const char*)qbuf[k]->p + (size_t)s * cap * v, (size_t)cap * v, hipMemcpyDeviceToHost));
            if (memcmp(back.data(), image[k].data(), (size_t)cap * v) != 0) out->queues_unchanged = 0u;
        }
    }
    // the occupied entries of the hit buffer, and their primitives: leaf order -> global primitive id
    float* const rec[1] = {out->hit4};
    out->hit_found = occupied_entries(1, &hit, qn, fill, cap, N, out->hit_place2, rec);
    std::vector<TriRec> tris(c->num_tris);
    HIPCHK(c, hipMemcpy(tris.data(), c->tris, sizeof(TriRec) * (size_t)c->num_tris, hipMemcpyDeviceToHost));
    for (size_t e = 0; e < N && e < (size_t)out->hit_found; e++) {
        uint32_t pos;
        memcpy(&pos, &out->hit4[4 * e + 3], 4);
        const bool miss = pos == 0xffffffffu;
        const size_t tri = miss ? 0 : (size_t)pos / 3;               // pos: offset in 16-byte units, a record is 48 bytes
        if (!miss && (pos % 3u != 0u || tri >= tris.size()))
            return fail(c, FOVPT_E_DEVICE, "%s: the hit record at (%u, %u) points at 16-byte unit %u", who, out->hit_place2[2 * e], out->hit_place2[2 * e + 1], pos);
        out->hit_prim[e] = miss ? 0xffffffffu : tris[tri].prim;
    }
    return FOVPT_OK;
}

}  // namespace

extern "C" {

// test/diagnostic hook: device address and size of an internal buffer
int fovpt_debug_buffer(fovpt_ctx* c, const char* name, void** ptr, size_t* bytes)
{
    if (!c || !name || !ptr || !bytes) return FOVPT_E_INVALID;
    if (strcmp(name, "bvh_nodes") == 0 && c->has_scene) { *ptr = c->nodes; *bytes = (size_t)c->stats.bvh_bytes; return FOVPT_OK; }   // tools/bvhstat.py
    if (strcmp(name, "bvh_tris") == 0 && c->has_scene) { *ptr = c->tris; *bytes = (size_t)c->stats.tri_bytes; return FOVPT_OK; }
    if (strcmp(name, "scene_vertices") == 0 && c->up_vtx.p) { *ptr = c->up_vtx.p; *bytes = c->h_vtx.size() * 4; return FOVPT_OK; }   // fovpt_update_vertices
    if (strcmp(name, "scene_vertices_prev") == 0 && c->vtx_prev.p) { *ptr = c->vtx_prev.p; *bytes = c->h_vtx.size() * 4; return FOVPT_OK; }   // fovpt_temporal_motion
    if (strcmp(name, "rig_world") == 0 && c->rig.set) { *ptr = c->rig.dev.world; *bytes = 48 * (size_t)c->rig.dev.num_nodes; return FOVPT_OK; }   // what k_rig_pose last wrote
    if (strcmp(name, "rig_rigid") == 0 && c->rig.set) { *ptr = c->rig.dev.rigid; *bytes = 48 * (size_t)c->rig.dev.num_rigid; return FOVPT_OK; }
    if (strcmp(name, "rig_palette") == 0 && c->rig.set) { *ptr = c->rig.dev.palette; *bytes = 48 * (size_t)c->rig.dev.num_pal; return FOVPT_OK; }
    if (strcmp(name, "post_color") == 0 && c->post.out.color.p) { *ptr = c->post.out.color.p; *bytes = c->post.out.color.bytes; return FOVPT_OK; }   // fovpt_post's own output, once made
    if (strcmp(name, "expose_histogram") == 0 && c->expose.hist.p) { *ptr = c->expose.hist.p; *bytes = FOVPT_EXPOSE_BINS * sizeof(uint64_t); return FOVPT_OK; }   // fovpt_expose's last metered step
    if (strcmp(name, "expose_state") == 0 && c->expose.state.p) { *ptr = c->expose.state.p; *bytes = sizeof(ExposeState); return FOVPT_OK; }
    if (strcmp(name, "bloom_pyramid") == 0 && c->bloom.pyramid.p) { *ptr = c->bloom.pyramid.p; *bytes = c->bloom.texels * 16; return FOVPT_OK; }   // fovpt_bloom's levels of the last call
    if (strcmp(name, "warp_keys") == 0 && c->warp.keys.p) { *ptr = c->warp.keys.p; *bytes = c->warp.keys.bytes; return FOVPT_OK; }   // fovpt_warp's keys, once made
    if (strcmp(name, "focus_state") == 0 && c->focus.state.p) { *ptr = c->focus.state.p; *bytes = sizeof(FocusState); return FOVPT_OK; }   // fovpt_focus's state record
    if (strcmp(name, "focus_scratch") == 0 && c->focus.rt.p) { *ptr = c->focus.rt.p; *bytes = c->focus.rt.bytes; return FOVPT_OK; }   // and its (r, tp) pairs, once made
    if (strcmp(name, "gbuffer_hit") == 0 && c->gbuffer.hit.p) { *ptr = c->gbuffer.hit.p; *bytes = c->gbuffer.pixels * 16; return FOVPT_OK; }   // the last G-buffer trace
    StateSet& S = c->engine.set[c->engine.rot.last_set];  // the set the most recent job used
    struct { const char* n; DevBuf* b; } tab[] = {
        {"sq_o", &S.sq_o[0]}, {"sq_d", &S.sq_d[0]}, {"sq_vis", &S.sq_vis[0]}, {"sq_occ", &S.sq_occ[0]}, {"counters", &S.counters},
        {"hit", &S.s_hit}, {"queue_a_o", &S.q_o[0]}, {"queue_a_d", &S.q_d[0]}, {"queue_b_o", &S.q_o[1]}, {"queue_b_d", &S.q_d[1]},
    };
    for (auto& t : tab)
        if (strcmp(t.n, name) == 0) { *ptr = t.b->p; *bytes = t.b->bytes; return FOVPT_OK; }
    return fail(c, FOVPT_E_INVALID, "unknown debug buffer %s", name);
}

// test hook: the PRODUCTION traversal kernel on a caller-supplied batch of rays -- closest hit (global primitive id, t, u, v)
// and the occlusion predicate of the shadow rays (any front-facing candidate in (0.01, 1e16), deviceProgram.cu:224-248,
// 284-300) -- so that optixTrace's two ray types can be compared with the oracle ray by ray, not only through frames.
int fovpt_debug_trace(fovpt_ctx* c, int n, const float* origins3, const float* dirs3, uint32_t* prim_out, float* tuv_out3, uint8_t* occluded_out)
{
    if (!c || n < 0 || (n && (!origins3 || !dirs3))) return FOVPT_E_INVALID;
    if (!c->has_scene) return fail(c, FOVPT_E_NO_SCENE, "fovpt_debug_trace without a scene");
    if (n == 0) return FOVPT_OK;
    // fovpt_debug_trace_queued with every ray in shard 0 of both queues, slot = index, cell 0, iteration 0 and the production grids
    const size_t un = (size_t)n, D = (size_t)c->cfg.max_depth;
    std::vector<uint32_t> slot(un), target(un, 0u), place(2 * un), prim(un);
    std::vector<float> vis(un * 4, 0.f), occ(un * 4, 0.f), hit(un * 4), cells((un + 1) * 4 * D), alpha((un + 1) * 4);
    for (size_t i = 0; i < un; i++) { slot[i] = (uint32_t)i; vis[4 * i] = 1.f; occ[4 * i] = 2.f; }      // what store_shadow leaves in the cell: 1 visible, 2 occluded
    fovpt_debug_trace_launch L;
    memset(&L, 0, sizeof(L));
    L.origins3 = origins3; L.dirs3 = dirs3; L.slot = slot.data(); L.target = target.data(); L.vis4 = vis.data(); L.occ4 = occ.data();
    L.n = n; L.q_count[0] = L.sq_count[0] = (uint32_t)n;
    fovpt_debug_trace_result R;
    memset(&R, 0, sizeof(R));
    R.hit_place2 = place.data(); R.hit4 = hit.data(); R.hit_prim = prim.data(); R.cells4 = cells.data(); R.alpha4 = alpha.data();
    CHK(trace_queued(c, &L, &R, "fovpt_debug_trace"));
    if (R.hit_found != (uint32_t)n) return fail(c, FOVPT_E_DEVICE, "fovpt_debug_trace: %u hit records for %d rays", R.hit_found, n);
    for (size_t i = 0; i < un; i++) {
        if (place[2 * i] != 0u || place[2 * i + 1] != (uint32_t)i) return fail(c, FOVPT_E_DEVICE, "fovpt_debug_trace: a hit record at (%u, %u)", place[2 * i], place[2 * i + 1]);
        if (prim_out) prim_out[i] = prim[i];
        if (tuv_out3) for (int k = 0; k < 3; k++) tuv_out3[3 * i + k] = hit[4 * i + k];
        if (occluded_out) {
            const float v = cells[4 * i * D];
            if (v != 1.f && v != 2.f) return fail(c, FOVPT_E_DEVICE, "shadow ray %zu left %g in its cell", i, (double)v);
            occluded_out[i] = v == 2.f ? 1 : 0;
        }
    }
    return FOVPT_OK;
}

// test hook: the PRODUCTION traversal launches on a caller-made queue state (include/fovpt.h), and everything they left
int fovpt_debug_trace_queued(fovpt_ctx* c, const fovpt_debug_trace_launch* launch, fovpt_debug_trace_result* out)
{
    return trace_queued(c, launch, out, "fovpt_debug_trace_queued");
}

// test hook: the PRODUCTION hierarchy build -- fovpt_build_lbvh itself, the function fovpt_set_scene and the rebuilds call -- over
// caller-supplied triangles under explicit switches, with a trace: what every stage left (fovpt_device.h, BvhBuildTrace).  The
// triangles, the hierarchy and the trace are the call's own: no member of the context changes but the error text.
int fovpt_debug_build(fovpt_ctx* c, uint32_t n, const float* tris9, const uint32_t* mesh_of_prim, const fovpt_debug_build_switches* sw,
                      fovpt_debug_build_trace* out)
{
    if (!c || !tris9 || !sw || !out || n == 0 || n > (1u << 24)) return FOVPT_E_INVALID;
    if (!(sw->split_budget >= 0.f) || sw->split_budget > 2.f || sw->reinsert_rounds < 0) return fail(c, FOVPT_E_INVALID, "fovpt_debug_build: switches out of range");
    CHK(debug_begin(c));
    DevBuf d_flat, d_mesh;
    HIPCHK(c, upload(d_flat, tris9, 36ull * n));
    HIPCHK(c, d_mesh.reserve(4ull * n));
    if (mesh_of_prim) HIPCHK(c, hipMemcpy(d_mesh.p, mesh_of_prim, 4ull * n, hipMemcpyHostToDevice));
    else HIPCHK(c, hipMemset(d_mesh.p, 0, 4ull * n));
    BvhSwitches bs;
    bs.use_ploc = sw->use_ploc ? 1 : 0; bs.split_budget = sw->split_budget; bs.order_children = sw->order_children ? 1 : 0;
    bs.reinsert_rounds = sw->reinsert_rounds; bs.verbose = 0;
    BvhBuildResult br;
    memset(&br, 0, sizeof(br));
    BvhBuildTrace T;
    char err[256];
    const hipError_t be = fovpt_build_lbvh(c->stream, (const float*)d_flat.p, (const uint32_t*)d_mesh.p, n, bs, sw->reinsert_rounds, &br, err, sizeof(err), &T);
    if (be != hipSuccess) return fail(c, FOVPT_E_DEVICE, "fovpt_debug_build: %s", err);
    struct Free { BvhBuildResult& b; ~Free() { free_hierarchy(b); } } free_nodes{br};     // (on every return below)
    const size_t R = br.num_refs, I = R - 1, N = br.num_nodes;
    out->num_refs = br.num_refs;
    if (R > out->cap_refs) return fail(c, FOVPT_E_INVALID, "fovpt_debug_build: %zu references, room for %u", R, out->cap_refs);
    if (T.round_end.size() > out->cap_rounds && out->round_end) return fail(c, FOVPT_E_INVALID, "fovpt_debug_build: %zu PLOC rounds, room for %u", T.round_end.size(), out->cap_rounds);
    if (br.num_levels == 0) return fail(c, FOVPT_E_INVALID, "fovpt_debug_build: the wide tree has more than %d levels", FOVPT_BVH_MAX_LEVELS);
    // every array of the trace has the length its stage gives it
    const bool tree = !T.tiny;
    const size_t want_i = tree ? I : 0;
    if (T.boxes.size() != 6 * R || T.vals_s.size() != R || T.leaf_pos.size() != R || T.nodes_pre.size() != 32 * N || T.keys_s.size() != (tree ? R : 0)
        || T.left0.size() != want_i || T.right0.size() != want_i || T.ibox0.size() != 6 * want_i || T.left1.size() != want_i || T.right1.size() != want_i
        || T.ibox1.size() != 6 * want_i || T.size_int.size() != want_i || T.node_first.size() != want_i || T.dp.size() != 4 * want_i
        || (!T.split_count.empty() && T.split_count.size() != n) || (T.splits && (T.split_first.size() != n || T.ref_prim.size() != R)))
        return fail(c, FOVPT_E_DEVICE, "fovpt_debug_build: a stage's arrays do not have the build's sizes");
    auto put = [](auto* dst, const auto& v) { if (dst && !v.empty()) memcpy(dst, v.data(), v.size() * sizeof(v[0])); };
    put(out->split_count, T.split_count); put(out->split_first, T.split_first); put(out->ref_prim, T.ref_prim);
    put(out->boxes, T.boxes); put(out->keys_s, T.keys_s); put(out->vals_s, T.vals_s);
    put(out->left0, T.left0); put(out->right0, T.right0); put(out->ibox0, T.ibox0); put(out->round_end, T.round_end);
    put(out->left1, T.left1); put(out->right1, T.right1); put(out->ibox1, T.ibox1);
    put(out->size_int, T.size_int); put(out->node_first, T.node_first); put(out->leaf_pos, T.leaf_pos); put(out->dp, T.dp);
    put(out->nodes_pre, T.nodes_pre);
    if (out->nodes) HIPCHK(c, hipMemcpy(out->nodes, br.nodes, sizeof(BvhNode4) * N, hipMemcpyDeviceToHost));
    if (out->tris) HIPCHK(c, hipMemcpy(out->tris, br.tris, sizeof(TriRec) * R, hipMemcpyDeviceToHost));
    out->tiny = (uint32_t)T.tiny; out->have_count = T.split_count.empty() ? 0u : 1u; out->have_splits = (uint32_t)T.splits;
    out->root = (uint32_t)T.root; out->num_rounds = (uint32_t)T.round_end.size();
    out->num_nodes = br.num_nodes; out->max_depth = br.max_depth; out->reinserted = br.reinserted; out->num_levels = br.num_levels;
    out->s_cut = T.s_cut;
    for (int a = 0; a < 6; a++) out->cbounds[a] = T.cbounds[a];
    for (uint32_t L = 0; L <= br.num_levels; L++) out->level_first[L] = br.level_first[L];
    return debug_end(c);
}

// test hook: the PRODUCTION shading kernel on caller-made hits -- one launch of fovpt_launch_shade (k_shade<false> or <true> by the
// configured options, as run_job launches it) over an input queue the caller laid out, and everything the kernel left: the slots'
// state, the counters and the occupied entries of the next radiance queue and of the shadow queue.  Every buffer the kernel may
// write is filled with the byte FOVPT_DEBUG_SHADE_FILL first, so that "not written" can be told from "written with zero".
int fovpt_debug_shade(fovpt_ctx* c, const fovpt_probe* probe, const fovpt_debug_shade_launch* in, const float* origin3, const float* dir4,
                      const uint32_t* prim, const float* tuv3, const uint32_t* rng3, const float* thr4, fovpt_debug_shade_result* out)
{
    if (!c || !probe || !in || !out || in->n < 0 || (in->n && (!origin3 || !dir4 || !prim || !tuv3 || !rng3 || !thr4))) return FOVPT_E_INVALID;
    if (!c->has_scene) return fail(c, FOVPT_E_NO_SCENE, "fovpt_debug_shade without a scene");
    if (!probe_complete(*probe)) return fail(c, FOVPT_E_NO_PROBE, "fovpt_debug_shade with an incomplete probe");
    const int n = in->n;
    if (in->sel > 2u || in->grid < 1 || in->grid > 4096 || in->depth_iter < 0 || in->depth_iter + 1 >= FOVPT_MAX_ITERS)
        return fail(c, FOVPT_E_INVALID, "fovpt_debug_shade: sel %u, grid %d, depth_iter %d", in->sel, in->grid, in->depth_iter);
    if (c->cfg.max_depth < 1 || c->cfg.max_depth > 32) return fail(c, FOVPT_E_INVALID, "max_depth out of range");
    if (c->cfg.write_guides && c->any_catcher) return fail(c, FOVPT_E_INVALID, "write_guides is not available with shadow-catcher materials");
    uint64_t total = 0;
    for (uint32_t s = 0; s < FOVPT_SHARDS; s++) {
        const bool selected = in->sel == 0u || (in->sel == 1u) == (s < 4u);
        if (in->shard_count[s] && !selected) return fail(c, FOVPT_E_INVALID, "fovpt_debug_shade: input in shard %u outside the selection %u", s, in->sel);
        total += in->shard_count[s];
    }
    if (total != (uint64_t)n) return fail(c, FOVPT_E_INVALID, "fovpt_debug_shade: the shards hold %llu inputs, n = %d", (unsigned long long)total, n);
    const size_t D = (size_t)c->cfg.max_depth, un = (size_t)n;
    const bool guides = c->cfg.write_guides != 0;
    if (n && (!out->rng4 || !out->thr4 || !out->rad4 || !out->alpha4 || (guides && (!out->guide_n4 || !out->guide_a4)) || !out->next_place2
              || !out->next_o4 || !out->next_d4 || !out->shadow_place2 || !out->shadow_o4 || !out->shadow_d4 || !out->shadow_vis4 || !out->shadow_occ4))
        return FOVPT_E_INVALID;
    const size_t slots = (un ? un : 1u) * FOVPT_SHARDS;             // any one shard can hold everything
    StateSet* set = nullptr; uint32_t cap = 0;
    CHK(debug_state(c, slots, 1, set, cap));
    StateSet& S = *set;
    hipStream_t st = c->stream;
    const size_t qn = (size_t)cap * FOVPT_SHARDS, v = 16;
    // leaf-order record of a primitive: the first one when spatial splits made several (the inverse of fovpt_debug_trace's map)
    std::vector<TriRec> tris(c->num_tris);
    HIPCHK(c, hipMemcpy(tris.data(), c->tris, sizeof(TriRec) * (size_t)c->num_tris, hipMemcpyDeviceToHost));
    uint32_t nprim = 0;
    for (const TriRec& T : tris) nprim = T.prim + 1u > nprim ? T.prim + 1u : nprim;
    std::vector<uint32_t> first(nprim, 0xffffffffu);
    for (size_t k = tris.size(); k-- > 0;) first[tris[k].prim] = (uint32_t)k;
    // the input queue: shard s holds the next shard_count[s] hits, in order; slot of hit i = i
    std::vector<float> qo(qn * 4, 0.f), qd(qn * 4, 0.f), hit(qn * 4, 0.f);
    std::vector<uint32_t> rng(un * 4, 0u);
    size_t i = 0;
    for (uint32_t s = 0; s < FOVPT_SHARDS; s++)
        for (uint32_t k = 0; k < in->shard_count[s]; k++, i++) {
            const size_t ph = (size_t)s * cap + k;
            const uint32_t slot = (uint32_t)i;
            for (int a = 0; a < 3; a++) { qo[4 * ph + a] = origin3[3 * i + a]; hit[4 * ph + a] = tuv3[3 * i + a]; }
            memcpy(&qo[4 * ph + 3], &slot, 4);
            for (int a = 0; a < 4; a++) qd[4 * ph + a] = dir4[4 * i + a];
            uint32_t tpos = 0xffffffffu;
            if (prim[i] != 0xffffffffu) {
                if (prim[i] >= nprim || first[prim[i]] == 0xffffffffu) return fail(c, FOVPT_E_INVALID, "fovpt_debug_shade: hit %zu names primitive %u", i, prim[i]);
                tpos = first[prim[i]] * 3u;                                   // offset in 16-byte units, a record is 48 bytes
            }
            memcpy(&hit[4 * ph + 3], &tpos, 4);
            rng[4 * i] = rng3[3 * i]; rng[4 * i + 1] = rng3[3 * i + 1]; rng[4 * i + 2] = rng3[3 * i + 2]; rng[4 * i + 3] = 0u;
        }
    const int fill = FOVPT_DEBUG_SHADE_FILL;
    HIPCHK(c, hipMemcpyAsync(S.q_o[0].p, qo.data(), qn * v, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(S.q_d[0].p, qd.data(), qn * v, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(S.s_hit.p, hit.data(), qn * v, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(S.s_rng.p, fill, slots * v, st));
    HIPCHK(c, hipMemsetAsync(S.s_thr.p, fill, slots * v, st));
    if (n) {
        HIPCHK(c, hipMemcpyAsync(S.s_rng.p, rng.data(), un * v, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(S.s_thr.p, thr4, un * v, hipMemcpyHostToDevice, st));
    }
    HIPCHK(c, hipMemsetAsync(S.s_rad.p, fill, slots * v * D, st));
    HIPCHK(c, hipMemsetAsync(S.s_alpha.p, fill, slots * v, st));
    if (guides) { HIPCHK(c, hipMemsetAsync(S.s_guide_n.p, fill, slots * v, st)); HIPCHK(c, hipMemsetAsync(S.s_guide_a.p, fill, slots * v, st)); }
    const DevBuf* const outq[6] = {&S.q_o[1], &S.q_d[1], &S.sq_o[0], &S.sq_d[0], &S.sq_vis[0], &S.sq_occ[0]};      // the next queue's o, d and the shadow queue's o, d, vis, occ
    for (const DevBuf* b : outq) HIPCHK(c, hipMemsetAsync(b->p, fill, qn * v, st));
    const int w_in = FOVPT_CNT_Q(in->depth_iter), w_next = FOVPT_CNT_Q(in->depth_iter + 1), w_shadow = FOVPT_CNT_SQ(in->depth_iter);
    std::vector<uint32_t> was(cnt_words, 0u), cw;
    for (uint32_t s = 0; s < FOVPT_SHARDS; s++) was[(size_t)s * FOVPT_SHARD_STRIDE + w_in] = in->shard_count[s];
    HIPCHK(c, put_counters(S, was, st));
    // what k_shade reads of a frame: the probe and how it is searched, the depth cap, the options, the partition
    FrameDev fd;
    memset(&fd, 0, sizeof(fd));
    fd.w = fd.h = 1;
    fd.probe = *probe;
    const ProbePath pp = probe_path(c, *probe);
    fd.guide_x = pp.guide_x; fd.guide_y = pp.guide_y; fd.probe_rec = pp.rec; fd.probe_row_mul = pp.row_mul;
    fd.max_depth = c->cfg.max_depth; fd.options = c->cfg.options; fd.partition = in->partition ? 1 : 0;
    fd.world = 1; fd.tile_w = 8; fd.tile_h = 4;
    fovpt_launch_shade(st, fd, scene_view(c), path_state(c, S), ray_queue(S, 0), ray_queue(S, 1), shadow_queue(S, 0), cap, (Counters*)S.counters.p,
                       in->depth_iter, in->grid, nullptr, in->sel);
    HIPCHK(c, hipGetLastError());
    std::vector<uint32_t> back[6];                                  // what outq holds afterwards
    if (n) {
        HIPCHK(c, hipMemcpyAsync(out->rng4, S.s_rng.p, un * v, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(out->thr4, S.s_thr.p, un * v, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(out->rad4, S.s_rad.p, un * v * D, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(out->alpha4, S.s_alpha.p, un * v, hipMemcpyDeviceToHost, st));
        if (guides) {
            HIPCHK(c, hipMemcpyAsync(out->guide_n4, S.s_guide_n.p, un * v, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipMemcpyAsync(out->guide_a4, S.s_guide_a.p, un * v, hipMemcpyDeviceToHost, st));
        }
    }
    for (int k = 0; k < 6; k++) { back[k].resize(qn * 4); HIPCHK(c, hipMemcpyAsync(back[k].data(), outq[k]->p, qn * v, hipMemcpyDeviceToHost, st)); }
    CHK(take_counters(c, S, cw, st));
    out->cap = cap;
    for (uint32_t s = 0; s < FOVPT_SHARDS; s++) {
        out->next_count[s] = cw[(size_t)s * FOVPT_SHARD_STRIDE + w_next];
        out->shadow_count[s] = cw[(size_t)s * FOVPT_SHARD_STRIDE + w_shadow];
    }
    out->counters_changed = counters_changed(cw, was, w_next, w_shadow);      // every other counter word is as it was
    // the occupied entries of both queues; at most n of each are handed out
    float* const next_rec[2] = {out->next_o4, out->next_d4};
    float* const shadow_rec[4] = {out->shadow_o4, out->shadow_d4, out->shadow_vis4, out->shadow_occ4};
    out->next_found = occupied_entries(2, back, qn, fill, cap, un, out->next_place2, next_rec);
    out->shadow_found = occupied_entries(4, back + 2, qn, fill, cap, un, out->shadow_place2, shadow_rec);
    return FOVPT_OK;
}

// test hook: the PRODUCTION resolve kernel on a caller-made path state.  The frame is the one a fovpt_launch (render = 0, a
// width x height grid) or a fovpt_render (render = 1: the passes of frame_passes) of these parameters would resolve (debug_frame),
// and the state of every sample slot and launch record is the caller's: what generate, shade and the occlusion launches would
// have left.  Called with state = NULL it only hands out the pass table, which the caller needs to lay the arrays out.  lp is
// not changed (a render's subframe_index is not advanced).
int fovpt_debug_resolve(fovpt_ctx* c, const fovpt_launch_params* lp, int render, uint32_t width, uint32_t height, fovpt_debug_pass* passes_out,
                        int* npass_out, const uint32_t* state, const float* cells4, const float* alpha4, const float* guide_n4, const float* guide_a4,
                        const float* backplate4, uint32_t* counters_left_out)
{
    if (!c || !lp || !passes_out || !npass_out) return FOVPT_E_INVALID;
    if (!lp->frame.accum_buffer || !lp->frame.frame_buffer) return fail(c, FOVPT_E_NO_FRAME, "fovpt_debug_resolve with null frame buffers");
    if (lp->frame.size.x <= 0 || lp->frame.size.y <= 0) return fail(c, FOVPT_E_INVALID, "bad frame size");
    if (c->cfg.max_depth < 1 || c->cfg.max_depth > 32) return fail(c, FOVPT_E_INVALID, "max_depth out of range");
    FrameDev fd;
    uint64_t slots = 0, launches = 0;
    CHK(debug_frame(c, lp, render, width, height, 0u, 0u, "fovpt_debug_resolve", fd, slots, launches, passes_out, npass_out));
    if (!state) return FOVPT_OK;
    if (counters_left_out) *counters_left_out = 0u;
    if (slots == 0) return FOVPT_OK;                                  // (a job of no sample slots launches nothing)
    if (!cells4 || !alpha4 || !backplate4 || (c->cfg.write_guides && (!guide_n4 || !guide_a4))) return FOVPT_E_INVALID;
    StateSet* set = nullptr; uint32_t cap = 0;
    CHK(debug_state(c, (size_t)slots, (size_t)launches, set, cap));
    StateSet& S = *set;
    hipStream_t st = c->stream;
    std::vector<uint32_t> rng((size_t)slots * 4, 0xdeadbeefu);        // the generator's words: nothing in a resolve reads them
    for (size_t i = 0; i < (size_t)slots; i++) rng[4 * i + 2] = state[i];
    const size_t v = 16, D = (size_t)c->cfg.max_depth;
    HIPCHK(c, hipMemcpyAsync(S.s_rng.p, rng.data(), (size_t)slots * v, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(S.s_rad.p, cells4, (size_t)slots * v * D, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(S.s_alpha.p, alpha4, (size_t)slots * v, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(S.s_backplate.p, backplate4, (size_t)launches * v, hipMemcpyHostToDevice, st));
    if (c->cfg.write_guides) {
        HIPCHK(c, hipMemcpyAsync(S.s_guide_n.p, guide_n4, (size_t)slots * v, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(S.s_guide_a.p, guide_a4, (size_t)slots * v, hipMemcpyHostToDevice, st));
    }
    // the queue sizes a job's launches leave behind, here a pattern: the resolve must leave zeros for the set's next job
    std::vector<uint32_t> left(cnt_words, 0xa5a5a5a5u);
    HIPCHK(c, put_counters(S, left, st));
    fovpt_launch_resolve(st, fd, path_state(c, S), (Counters*)S.counters.p);       // as run_job launches it
    HIPCHK(c, hipGetLastError());
    CHK(take_counters(c, S, left, st));          // (zeros from here on, whatever the kernel did)
    uint32_t nonzero = 0;
    for (uint32_t w : left) nonzero += w != 0u;
    if (counters_left_out) *counters_left_out = nonzero;
    return FOVPT_OK;
}

// test hook: the PRODUCTION generate launcher (fovpt_launch_generate: k_generate, or k_generate_owned for a rank of a sharded
// frame) on the frame a fovpt_launch (render = 0; with row1 > 0 the chunk [row0, row1) of it, as run_passes hands a chunk to
// run_job) or a fovpt_render (render = 1) of these parameters would run (debug_frame), and everything the launch left: the
// generator words, the backplates, the guides, the queue counters and the occupied entries of queue 0.
// The state is a job's (ensure_state, shard_capacity) except queue 0: the launch gets a scratch queue of 8 * cap + slots + 256
// entries with the same cap, so that a shard that overflows lands in memory this function owns and shows in the result (the
// appends of one launch number at most `slots`, and the last shard begins at 7 * cap).  Everything the kernel may write is
// filled with the byte FOVPT_DEBUG_SHADE_FILL first.  lp is not changed.
int fovpt_debug_generate(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_debug_generate_launch* in, fovpt_debug_pass* passes_out,
                         int* npass_out, fovpt_debug_generate_result* out)
{
    if (!c || !lp || !in || !passes_out || !npass_out) return FOVPT_E_INVALID;
    if (!lp->frame.accum_buffer || !lp->frame.frame_buffer) return fail(c, FOVPT_E_NO_FRAME, "fovpt_debug_generate with null frame buffers");
    if (!probe_complete(lp->probe)) return fail(c, FOVPT_E_NO_PROBE, "fovpt_debug_generate with an incomplete probe");
    if (lp->frame.size.x <= 0 || lp->frame.size.y <= 0) return fail(c, FOVPT_E_INVALID, "bad frame size");
    if (c->cfg.max_depth < 1 || c->cfg.max_depth > 32) return fail(c, FOVPT_E_INVALID, "max_depth out of range");
    const bool chunk = !in->render && in->row1 > 0u;
    if (in->render ? (in->row0 || in->row1) : (chunk && (in->row0 >= in->row1 || in->row1 > in->height)))
        return fail(c, FOVPT_E_INVALID, "fovpt_debug_generate: launch rows [%u, %u) of %u", in->row0, in->row1, in->height);
    FrameDev fd;
    uint64_t slots = 0, launches = 0;
    CHK(debug_frame(c, lp, in->render, in->width, in->height, in->row0, in->row1, "fovpt_debug_generate", fd, slots, launches, passes_out, npass_out));
    if (!out) return FOVPT_OK;
    // the launch: what run_job would give a launch of this `sel`, unless the caller says otherwise
    const uint32_t sel = in->sel;
    if (sel > 2u) return fail(c, FOVPT_E_INVALID, "fovpt_debug_generate: sel %u", sel);
    const int grid = in->grid ? in->grid : (sel ? c->engine.grid / 2 : c->engine.grid);
    if (grid <= 0 || grid > (1 << 20) || grid % (sel ? FOVPT_SHARDS / 2 : FOVPT_SHARDS))
        return fail(c, FOVPT_E_INVALID, "fovpt_debug_generate: a grid of %d blocks (a positive multiple of %d)", grid, sel ? FOVPT_SHARDS / 2 : FOVPT_SHARDS);
    uint32_t slot_begin = in->slot_begin, slot_end = in->slot_end;
    if (slot_begin == 0u && slot_end == 0u) {
        slot_end = (uint32_t)slots;
        if (sel) { const ChainSplit cs = chain_split(slots, (int)sel - 1); slot_begin = cs.slot_begin; slot_end = cs.slot_end; }
    }
    if (slot_begin > slot_end || (uint64_t)slot_end > slots) return fail(c, FOVPT_E_INVALID, "fovpt_debug_generate: sample slots [%u, %u) of %llu", slot_begin, slot_end, (unsigned long long)slots);
    const bool guides = c->cfg.write_guides != 0;
    out->found = out->counters_changed = 0u; out->kernel = 0u; out->guides = guides ? 1u : 0u;
    out->cap = shard_capacity((size_t)slots); out->slot_begin = slot_begin; out->slot_end = slot_end; out->grid = (uint32_t)grid;
    for (uint32_t s = 0; s < FOVPT_SHARDS; s++) out->count[s] = 0u;
    if (slots == 0) return FOVPT_OK;                                  // (a job of no sample slots launches nothing)
    if (!out->rng4 || !out->backplate4 || (guides && (!out->guide_n4 || !out->guide_a4)) || !out->place2 || !out->o4 || !out->d4) return FOVPT_E_INVALID;
    StateSet* set = nullptr; uint32_t cap = 0;
    CHK(debug_state(c, (size_t)slots, (size_t)launches, set, cap));
    StateSet& S = *set;
    hipStream_t st = c->stream;
    const size_t v = 16, qn = (size_t)cap * FOVPT_SHARDS + (size_t)slots + 256u;
    struct Scratch { void *o = nullptr, *d = nullptr; ~Scratch() { if (o) (void)hipFree(o); if (d) (void)hipFree(d); } } scratch;      // freed on every return path
    HIPCHK(c, hipMalloc(&scratch.o, qn * v)); HIPCHK(c, hipMalloc(&scratch.d, qn * v));
    const int fill = FOVPT_DEBUG_SHADE_FILL;
    HIPCHK(c, hipMemsetAsync(S.s_rng.p, fill, (size_t)slots * v, st));
    HIPCHK(c, hipMemsetAsync(S.s_backplate.p, fill, (size_t)launches * v, st));
    if (guides) { HIPCHK(c, hipMemsetAsync(S.s_guide_n.p, fill, (size_t)slots * v, st)); HIPCHK(c, hipMemsetAsync(S.s_guide_a.p, fill, (size_t)slots * v, st)); }
    HIPCHK(c, hipMemsetAsync(scratch.o, fill, qn * v, st)); HIPCHK(c, hipMemsetAsync(scratch.d, fill, qn * v, st));
    const std::vector<uint32_t> was(cnt_words, 0u);                   // as a job finds them
    HIPCHK(c, put_counters(S, was, st));
    RayQueue q0;
    q0.o = (float4*)scratch.o; q0.d = (float4*)scratch.d;
    out->kernel = (uint32_t)fovpt_launch_generate(st, fd, path_state(c, S), q0, cap, (Counters*)S.counters.p, slot_begin, slot_end, grid, sel);   // as run_job launches it
    HIPCHK(c, hipGetLastError());
    std::vector<uint32_t> q[2], cw;                                   // the scratch queue's o, d
    for (auto& a : q) a.resize(qn * 4);
    HIPCHK(c, hipMemcpyAsync(out->rng4, S.s_rng.p, (size_t)slots * v, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(out->backplate4, S.s_backplate.p, (size_t)launches * v, hipMemcpyDeviceToHost, st));
    if (guides) {
        HIPCHK(c, hipMemcpyAsync(out->guide_n4, S.s_guide_n.p, (size_t)slots * v, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(out->guide_a4, S.s_guide_a.p, (size_t)slots * v, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(c, hipMemcpyAsync(q[0].data(), scratch.o, qn * v, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(q[1].data(), scratch.d, qn * v, hipMemcpyDeviceToHost, st));
    CHK(take_counters(c, S, cw, st));
    for (uint32_t s = 0; s < FOVPT_SHARDS; s++) out->count[s] = cw[(size_t)s * FOVPT_SHARD_STRIDE + FOVPT_CNT_Q(0)];
    out->counters_changed = counters_changed(cw, was, FOVPT_CNT_Q(0), -1);
    // the occupied entries of the scratch queue (an entry of the guard region behind the eight shards reports a shard of 8 or
    // more); at most `slots` are handed out
    float* const rec[2] = {out->o4, out->d4};
    out->found = occupied_entries(2, q, qn, fill, cap, slots, out->place2, rec);
    return FOVPT_OK;
}

int fovpt_debug_probe_sample(fovpt_ctx* c, const fovpt_probe* probe, int flags, int n, const float* r12, int32_t* rowcol_out2, float* out7, int* path_out)
{
    CHK(debug_probe_args(c, probe, flags, n, r12, "fovpt_debug_probe_sample"));
    // Randf's range (maths.h:199-210): what the searches may be handed
    for (size_t i = 0; i < 2 * (size_t)n; i++)
        if (!(r12[i] >= 0.0f && r12[i] <= 0.999999f)) return fail(c, FOVPT_E_INVALID, "fovpt_debug_probe_sample: number %zu (%g) is outside [0, 0.999999]", i, (double)r12[i]);
    const ProbePath pp = debug_probe_path(c, *probe, flags, path_out);
    if (n == 0) return FOVPT_OK;
    CHK(debug_begin(c));
    DevBuf in, rowcol, out;
    HIPCHK(c, upload(in, r12, (size_t)n * 8)); HIPCHK(c, rowcol.reserve((size_t)n * 8)); HIPCHK(c, out.reserve((size_t)n * 28));
    fovpt_launch_debug_probe_sample(c->stream, *probe, pp.guide_x, pp.guide_y, pp.rec, pp.row_mul, n, (const float2*)in.p, (int2*)rowcol.p, (float*)out.p);
    CHK(debug_end(c));
    HIPCHK(c, download(rowcol_out2, rowcol, (size_t)n * 8)); HIPCHK(c, download(out7, out, (size_t)n * 28));
    return FOVPT_OK;
}

int fovpt_debug_probe_eval(fovpt_ctx* c, const fovpt_probe* probe, int flags, int n, const float* dirs3, float* out6, int* path_out)
{
    CHK(debug_probe_args(c, probe, flags, n, dirs3, "fovpt_debug_probe_eval"));
    const ProbePath pp = debug_probe_path(c, *probe, flags, path_out);
    if (n == 0) return FOVPT_OK;
    CHK(debug_begin(c));
    DevBuf in, out;
    HIPCHK(c, upload(in, dirs3, (size_t)n * 12)); HIPCHK(c, out.reserve((size_t)n * 24));
    fovpt_launch_debug_probe_eval(c->stream, *probe, pp.row_mul, n, (const float*)in.p, (float*)out.p);
    CHK(debug_end(c));
    HIPCHK(c, download(out6, out, (size_t)n * 24));
    return FOVPT_OK;
}

int fovpt_debug_bsdf(fovpt_ctx* c, const fovpt_material* material, int n, const float* N3, const float* view3, const float* albedo3, const float* etaI,
                     const float* etaO, const int32_t* seeds, const float* L_given3, float* out14)
{
    if (!c || !material || n < 0 || (n && (!N3 || !view3 || !albedo3 || !etaI || !etaO || !seeds || !L_given3))) return FOVPT_E_INVALID;
    if (n == 0) return FOVPT_OK;
    CHK(debug_begin(c));
    std::vector<float> rows((size_t)n * 16, 0.f), res((size_t)n * 16);
    for (int i = 0; i < n; i++) {
        float* r = &rows[16 * (size_t)i];
        for (int k = 0; k < 3; k++) { r[k] = N3[3 * (size_t)i + k]; r[3 + k] = view3[3 * (size_t)i + k]; r[6 + k] = albedo3[3 * (size_t)i + k]; r[12 + k] = L_given3[3 * (size_t)i + k]; }
        r[9] = etaI[i]; r[10] = etaO[i];
        memcpy(&r[11], &seeds[i], 4);
    }
    DevBuf in, out;
    HIPCHK(c, upload(in, rows.data(), (size_t)n * 64)); HIPCHK(c, out.reserve((size_t)n * 64));
    fovpt_launch_debug_bsdf(c->stream, *material, n, (const float*)in.p, (float*)out.p);
    CHK(debug_end(c));
    HIPCHK(c, download(res.data(), out, (size_t)n * 64));
    if (out14) for (int i = 0; i < n; i++) memcpy(out14 + 14 * (size_t)i, &res[16 * (size_t)i], 56);
    return FOVPT_OK;
}

int fovpt_debug_tex2d(fovpt_ctx* c, int texture, int n, const float* uv2, float* rgba_out4)
{
    if (!c || n < 0 || (n && !uv2)) return FOVPT_E_INVALID;
    if (!c->has_scene) return fail(c, FOVPT_E_NO_SCENE, "fovpt_debug_tex2d without a scene");
    if (texture < 0 || (size_t)texture >= c->tex_pixels.size()) return fail(c, FOVPT_E_INVALID, "fovpt_debug_tex2d: texture %d of %zu", texture, c->tex_pixels.size());
    if (n == 0) return FOVPT_OK;
    CHK(debug_begin(c));
    DevBuf in, out;
    HIPCHK(c, upload(in, uv2, (size_t)n * 8)); HIPCHK(c, out.reserve((size_t)n * 16));
    fovpt_launch_debug_tex2d(c->stream, (const TexDev*)c->textures.p, texture, n, (const float2*)in.p, (float4*)out.p);
    CHK(debug_end(c));
    HIPCHK(c, download(rgba_out4, out, (size_t)n * 16));
    return FOVPT_OK;
}

int fovpt_debug_math(fovpt_ctx* c, int op, const float* a, const float* b, float* out, size_t n)
{
    if (!c || !a || !out) return FOVPT_E_INVALID;
    if (n == 0) return FOVPT_OK;
    CHK(debug_begin(c));
    DevBuf ba, bb, bo;
    HIPCHK(c, upload(ba, a, n * 4)); HIPCHK(c, b ? upload(bb, b, n * 4) : bb.reserve(n * 4)); HIPCHK(c, bo.reserve(n * 4));
    if (!b) HIPCHK(c, hipMemset(bb.p, 0, n * 4));
    fovpt_launch_math(c->stream, op, (const float*)ba.p, (const float*)bb.p, (float*)bo.p, n);
    CHK(debug_end(c));
    HIPCHK(c, download(out, bo, n * 4));
    return FOVPT_OK;
}

}  // extern "C"
