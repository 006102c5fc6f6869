// api_post.hip -- post-processing of the rendered frame over the C ABI, first half: the steps every post-frame stage shares (declared
// in fovpt_ctx.h; api_view.hip and api_packet.hip use them too), what fovpt_resize and fovpt_set_scene ask of the stages
// (post_resize, post_scene_changed), and the stages that rebuild the image: fovpt_denoise (denoise.hip), fovpt_gbuffer /
// fovpt_reconstruct (reconstruct.hip), fovpt_temporal / fovpt_temporal_motion (temporal.hip), fovpt_post (post_fused.hip),
// fovpt_variance / fovpt_variance_filter (variance.hip), fovpt_bloom (bloom.hip), and their defaults.  Every stage has the same parts -- *_check (nothing
// allocated, enqueued or changed), the kernel's arguments from the config and the rendered frame's record (*_args where more than
// one place needs them) and *_enqueue (reservations and launches of a checked call; the two variance calls, which nothing else
// enqueues, have theirs in the entry point) -- and its entry point is: null checks, check, hipSetDevice, own outputs, alias check,
// enqueue.  fovpt_post checks every enabled stage, then enqueues them.  The state is fovpt_ctx::rendered and one struct per stage
// (fovpt_ctx.h).
#include <cmath>
#include <cstring>

#include "fovpt_camera.h"
#include "fovpt_ctx.h"

// ---- the shared steps ----------------------------------------------------------------------------------------------------------

// What a post-frame stage, the quality metric and the packet encoder (`who`) ask of the frame last rendered: there is one, it has
// the guides where the call needs them (need_guides: the error text, or null), it is not a tile shard (a shard has no neighbours
// `to_what`; null: the caller needs the whole frame for another reason), lp's frame has its size, and that is fewer than `limit`
// pixels (0: any number).
int check_rendered_frame(fovpt_ctx* c, const fovpt_launch_params* lp, const char* who, const char* to_what, const char* need_guides, size_t limit)
{
    const fovpt_ctx::Rendered& R = c->rendered;
    if (R.w <= 0 || R.h <= 0) return fail(c, FOVPT_E_NO_FRAME, "%s: no frame rendered yet", who);
    if (need_guides && (!R.guides || c->any_catcher)) return fail(c, FOVPT_E_INVALID, "%s", need_guides);
    if (R.world > 1 && to_what) return fail(c, FOVPT_E_INVALID, "%s: a tile shard (world = %d) has no neighbours to %s", who, R.world, to_what);
    if (R.world > 1) return fail(c, FOVPT_E_INVALID, "%s: a tile shard (world = %d) does not see the frame", who, R.world);
    if (lp->frame.size.x != R.w || lp->frame.size.y != R.h)
        return fail(c, FOVPT_E_NO_FRAME, "%s: frame size %d x %d differs from the last frame's %d x %d", who, lp->frame.size.x, lp->frame.size.y, R.w, R.h);
    if (limit && R.pixels() >= limit) return fail(c, FOVPT_E_INVALID, "%s: frame too large (%d x %d)", who, R.w, R.h);
    return FOVPT_OK;
}

int check_reserved(fovpt_ctx* c, const int32_t* words, int n, const char* who)
{
    for (int k = 0; k < n; k++)
        if (words[k] != 0) return fail(c, FOVPT_E_INVALID, "%s: reserved fields must be 0", who);
    return FOVPT_OK;
}

// No output (a null one is not written) is an input of the call -- fmt_input: the error text, which says why -- or an earlier output.
int check_aliases(fovpt_ctx* c, std::initializer_list<const void*> outs, std::initializer_list<const void*> ins, const char* who, const char* fmt_input)
{
    for (const void* const* o = outs.begin(); o != outs.end(); o++) {
        if (!*o) continue;
        for (const void* p : ins)
            if (p == *o) return fail(c, FOVPT_E_INVALID, fmt_input, who);
        for (const void* const* q = outs.begin(); q != o; q++)
            if (*q == *o) return fail(c, FOVPT_E_INVALID, "%s: two outputs are the same buffer", who);
    }
    return FOVPT_OK;
}

// The rows of [U V W]^-1, each entry rounded to binary32 (fovpt_camera.h, which packet_host.cpp shares).  false: det is 0 or not finite.
bool camera_inverse(const float* U, const float* V, const float* W, float* inv) { return fovpt_camera_inverse(U, V, W, inv); }

// The G-buffer a caller gave, or with none the context's own (null pointers until the first trace)
GBufferDev gbuffer_dev(const fovpt_ctx* c, const fovpt_gbuffer_ptrs* given)
{
    const fovpt_ctx::GBuffer& G = c->gbuffer;
    GBufferDev g;
    if (given) { g.prim = given->prim; g.pos = (float4*)given->position; g.nrm = (float4*)given->normal; g.alb = (float4*)given->albedo; }
    else { g.prim = (uint32_t*)G.prim.p; g.pos = (float4*)G.pos.p; g.nrm = (float4*)G.nrm.p; g.alb = (float4*)G.alb.p; }
    return g;
}

static void gbuffer_ptrs(const GBufferDev& g, int w, int h, fovpt_gbuffer_ptrs* out)
{
    out->prim = g.prim;
    out->position = (fovpt_float4*)g.pos; out->normal = (fovpt_float4*)g.nrm; out->albedo = (fovpt_float4*)g.alb;
    out->width = w; out->height = h;
}

// The caller gave no output, or asks for the context's own (the *_buffers calls): the colour / rgba pair of the last frame's
// size, made on first use, for whichever of the two is null.
int own_outputs(fovpt_ctx* c, const char* who, OutPair& own, fovpt_float4*& out_color, uint32_t*& out_rgba)
{
    if (out_color && out_rgba) return FOVPT_OK;
    if (!own.color.p) {
        if (c->rendered.w <= 0 || c->rendered.h <= 0) return fail(c, FOVPT_E_NO_FRAME, "%s: no frame rendered yet", who);
        HIPCHK(c, hipSetDevice(c->device));
    }
    HIPCHK(c, own.reserve(c->rendered.pixels()));
    if (!out_color) out_color = (fovpt_float4*)own.color.p;
    if (!out_rgba) out_rgba = (uint32_t*)own.rgba.p;
    return FOVPT_OK;
}

// the body of a fovpt_*_buffers entry point (c is not null)
int own_buffers(fovpt_ctx* c, const char* who, OutPair& own, fovpt_float4** color, uint32_t** rgba)
{
    if (!color || !rgba) return FOVPT_E_INVALID;
    *color = nullptr; *rgba = nullptr;
    return own_outputs(c, who, own, *color, *rgba);
}

// A record the device keeps for a stage (a state, a set of counts): made zeroed on first use ...
int record_make(fovpt_ctx* c, DevBuf& rec, size_t bytes)
{
    if (rec.p) return FOVPT_OK;
    HIPCHK(c, rec.reserve(bytes));
    HIPCHK(c, hipMemset(rec.p, 0, bytes));
    return FOVPT_OK;
}

// ... zeroed again on st, or with st null now (no record yet: it will be made that way) ...
int record_reset(fovpt_ctx* c, DevBuf& rec, size_t bytes, hipStream_t st)
{
    if (!rec.p) return FOVPT_OK;
    if (st) HIPCHK(c, hipMemsetAsync(rec.p, 0, bytes, st));
    else HIPCHK(c, hipMemset(rec.p, 0, bytes));
    return FOVPT_OK;
}

// ... and read behind everything enqueued on fovpt_stream(); zeros while there is none (null_text: the error text for a null `out`)
int record_read(fovpt_ctx* c, const DevBuf& rec, void* out, size_t bytes, const char* null_text)
{
    if (!out) return fail(c, FOVPT_E_INVALID, null_text);
    memset(out, 0, bytes);
    if (!rec.p) return FOVPT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->shadow_stream));
    HIPCHK(c, hipMemcpy(out, rec.p, bytes, hipMemcpyDeviceToHost));
    return FOVPT_OK;
}

// the G-buffer's buffers for n pixels (the counters once: k_gbuffer_rays rewrites the queue sizes it uses on every call)
static int reserve_gbuffer(fovpt_ctx* c, size_t n)
{
    fovpt_ctx::GBuffer& G = c->gbuffer;
    HIPCHK(c, G.o.reserve(n * 16)); HIPCHK(c, G.d.reserve(n * 16)); HIPCHK(c, G.hit.reserve(n * 16));
    HIPCHK(c, G.prim.reserve(n * 4)); HIPCHK(c, G.pos.reserve(n * 16)); HIPCHK(c, G.nrm.reserve(n * 16)); HIPCHK(c, G.alb.reserve(n * 16));
    return record_make(c, G.cnt, sizeof(Counters));
}

// fovpt_temporal's G-buffer sets, histories and outputs for n pixels
static int reserve_temporal(fovpt_ctx* c, size_t n)
{
    fovpt_ctx::Temporal& T = c->temporal;
    for (int k = 0; k < 2; k++) {
        HIPCHK(c, T.prim[k].reserve(n * 4)); HIPCHK(c, T.pos[k].reserve(n * 16)); HIPCHK(c, T.nrm[k].reserve(n * 16));
        HIPCHK(c, T.alb[k].reserve(n * 16)); HIPCHK(c, T.hist[k].reserve(n * 16));
    }
    HIPCHK(c, T.out.reserve(n));
    return FOVPT_OK;
}

// fovpt_variance's moment histories and variance image for n pixels
static int reserve_variance(fovpt_ctx* c, size_t n)
{
    fovpt_ctx::Variance& V = c->variance;
    HIPCHK(c, V.hist[0].reserve(n * 16)); HIPCHK(c, V.hist[1].reserve(n * 16)); HIPCHK(c, V.image.reserve(n * 16));
    return FOVPT_OK;
}

// the texels of fovpt_bloom's pyramid for a w x h frame, with every level a call may ask for
static size_t bloom_pyramid_texels(int w, int h)
{
    int W, H;
    size_t end;
    fovpt_bloom_level(w, h, FOVPT_BLOOM_MAX_LEVELS, &W, &H, &end);
    return end;
}

// fovpt_resize: what exists of the stages' buffers follows the frame (nothing is made here); the states of fovpt_expose and
// fovpt_focus and the record of fovpt_quality stay
int post_resize(fovpt_ctx* c, int w, int h)
{
    const size_t n = (size_t)w * h;
    auto follow = [n](OutPair& own) { return own.color.p ? own.reserve(n) : hipSuccess; };
    HIPCHK(c, follow(c->denoise.out));
    if (c->gbuffer.prim.p) CHK(reserve_gbuffer(c, n));
    HIPCHK(c, follow(c->reconstruct.out));
    if (c->temporal.hist[0].p) CHK(reserve_temporal(c, n));
    HIPCHK(c, follow(c->post.out));
    HIPCHK(c, follow(c->expose.out));
    HIPCHK(c, follow(c->bloom.out));
    if (c->bloom.pyramid.p) HIPCHK(c, c->bloom.pyramid.reserve(bloom_pyramid_texels(w, h) * 16));
    c->bloom.texels = 0;                                                   // (the levels in it are of another size)
    if (c->warp.keys.p) HIPCHK(c, c->warp.keys.reserve(n * 8));
    if (c->warp.out.color.p) HIPCHK(c, c->warp.out.color.reserve(n * 16));     // (a warp of one image makes only that one)
    if (c->warp.out.rgba.p) HIPCHK(c, c->warp.out.rgba.reserve(n * 4));
    if (c->focus.rt.p) HIPCHK(c, c->focus.rt.reserve(n * 8));
    HIPCHK(c, follow(c->focus.out));
    HIPCHK(c, follow(c->lens.out));
    if (c->variance.hist[0].p) CHK(reserve_variance(c, n));
    HIPCHK(c, follow(c->variance.out));
    c->variance.valid = false;                                             // (its history is of another size, and so is its image)
    c->variance.own_w = c->variance.own_h = 0;
    if (c->quality.rows.p) HIPCHK(c, c->quality.rows.reserve((size_t)fovpt_quality_rows(w, h) * FOVPT_QUALITY_COLUMNS * sizeof(uint64_t)));
    c->temporal.valid = false;                                             // (its history is of another size)
    c->rendered.w = c->rendered.h = 0;                                     // (nothing rendered at this size yet)
    c->seq_frame = ++c->seq;                                               // (fovpt_warp_motion: nor traced)
    return FOVPT_OK;
}

int post_scene_changed(fovpt_ctx* c)
{
    c->temporal.valid = false;                       // fovpt_temporal's history: primitive ids change
    c->variance.valid = false;                       // fovpt_variance's moments: of another scene's surfaces
    c->seq_frame = ++c->seq;                         // fovpt_warp_motion: the hit records of the last trace are another scene's
    CHK(record_reset(c, c->expose.state, sizeof(ExposeState), nullptr));   // fovpt_expose adapts to another scene from scratch
    return record_reset(c, c->focus.state, sizeof(FocusState), nullptr);   // and fovpt_focus meters it from scratch
}

// Enqueues the G-buffer of lp's frame.size seen by view's camera (view.eye / U / V / W) on fovpt_stream(): one ray per pixel,
// traced by the production closest-hit k_traverse (so a ray gets the (prim, t, u, v) fovpt_debug_trace returns for it), then
// the per-pixel outputs: into target's buffers (frame.size entries each), or with target null into the ones fovpt_gbuffer
// hands out.  The ray queue, hit records and counters are shared: every use is ordered on the same stream.
int enqueue_gbuffer(fovpt_ctx* c, const fovpt_launch_params* lp, const FrameDev& view, GBufferDev& g, const char* who,
                    const GBufferDev* target)
{
    if (!c->has_scene || lp->traversable != c->scene_id) return fail(c, FOVPT_E_NO_SCENE, "%s without a scene (traversable %llu, current %llu)", who,
                                                                     (unsigned long long)lp->traversable, (unsigned long long)c->scene_id);
#if FOVPT_V_STEPSTAT
    return fail(c, FOVPT_E_INVALID, "%s: not available in a diagnostic (FOVPT_V_STEPSTAT) build", who);
#endif
    const int w = lp->frame.size.x, h = lp->frame.size.y;
    if (w <= 0 || h <= 0) return fail(c, FOVPT_E_INVALID, "%s: frame size %d x %d", who, w, h);
    const size_t n = (size_t)w * (size_t)h;
    if (n >= (1ull << 31)) return fail(c, FOVPT_E_INVALID, "%s: frame too large (%d x %d)", who, w, h);
    HIPCHK(c, hipSetDevice(c->device));
    c->gb_stamp = 0;
    CHK(reserve_gbuffer(c, n));
    fovpt_ctx::GBuffer& G = c->gbuffer;
    const fovpt_ctx::Rendered& R = c->rendered;
    G.pixels = n;
    // fovpt_warp_motion: whose hit records these are -- the rendered frame's when this is its size and camera
    if (w == R.w && h == R.h && !memcmp(view.eye, R.frame.eye, sizeof(view.eye)) && !memcmp(view.U, R.frame.U, sizeof(view.U)) &&
        !memcmp(view.V, R.frame.V, sizeof(view.V)) && !memcmp(view.W, R.frame.W, sizeof(view.W)))
        c->gb_stamp = ++c->seq;
    FrameDev fd;
    memset(&fd, 0, sizeof(fd));
    fd.w = w; fd.h = h;
    memcpy(fd.eye, view.eye, sizeof(fd.eye)); memcpy(fd.U, view.U, sizeof(fd.U));
    memcpy(fd.V, view.V, sizeof(fd.V)); memcpy(fd.W, view.W, sizeof(fd.W));
    RayQueue q; q.o = (float4*)G.o.p; q.d = (float4*)G.d.p;
    PathState ps;
    memset(&ps, 0, sizeof(ps));
    ps.hit = (float4*)G.hit.p;                                       // all a closest-hit launch writes
    ShadowQueue sq;
    memset(&sq, 0, sizeof(sq));
    Counters* cnt = (Counters*)G.cnt.p;
    g = target ? *target : gbuffer_dev(c, nullptr);
    hipStream_t st = c->shadow_stream;
    fovpt_launch_gbuffer_rays(st, fd, q, cnt);
    fovpt_launch_traverse(st, scene_view(c), ps, q, sq, (uint32_t)n, cnt, 0, -1, c->engine.grid_trace);   // shard 0 holds all n rays
    fovpt_launch_gbuffer_fill(st, fd, scene_view(c), q, ps.hit, g);
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

namespace {

float inv_sq(float s) { const float s2 = s * s; return 1.0f / s2; }

GBufferDev temporal_set(const fovpt_ctx* c, int k)
{
    const fovpt_ctx::Temporal& T = c->temporal;
    GBufferDev g;
    g.prim = (uint32_t*)T.prim[k].p; g.pos = (float4*)T.pos[k].p; g.nrm = (float4*)T.nrm[k].p; g.alb = (float4*)T.alb[k].p;
    return g;
}

// ---- what the entry points and fovpt_post share: per stage its validation (nothing allocated, enqueued or changed), its kernel
// arguments, and its launches ----------------------------------------------------------------------------------------------

// fovpt_denoise's validation
int denoise_check(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_denoise_config* dc, const char* who)
{
    const int32_t its[4] = {dc->iterations_fovea, dc->iterations_middle, dc->iterations_periphery, dc->iterations_uniform};
    for (int32_t n : its)
        if (n < 0 || n > FOVPT_DENOISE_MAX_ITERATIONS) return fail(c, FOVPT_E_INVALID, "%s: iteration count %d outside 0 .. %d", who, n, FOVPT_DENOISE_MAX_ITERATIONS);
    const float sig[3] = {dc->color_sigma, dc->normal_sigma, dc->albedo_sigma};
    for (float v : sig)
        if (!sigma_ok(v)) return fail(c, FOVPT_E_INVALID, "%s: sigma %g outside [%g, %g]", who, (double)v, (double)FOVPT_SIGMA_MIN, (double)FOVPT_SIGMA_MAX);
    CHK(check_rendered_frame(c, lp, who, "filter with", "fovpt_denoise needs the denoiser guides: the frame was rendered without fovpt_config.write_guides = 1 (not available with shadow-catcher materials)", 0));
    if (!lp->frame.color_buffer || !lp->frame.normal_buffer || !lp->frame.albedo_buffer) return fail(c, FOVPT_E_INVALID, "%s: null guide buffers", who);
    return FOVPT_OK;
}

// the denoiser's buffers and launches for a checked call; out_color / out_rgba are set
int denoise_enqueue(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_denoise_config* dc, fovpt_float4* out_color, uint32_t* out_rgba)
{
    const size_t npix = c->rendered.pixels();
    HIPCHK(c, c->denoise.level.reserve(npix));
    HIPCHK(c, c->denoise.i0.reserve(npix * 16));
    HIPCHK(c, c->denoise.i1.reserve(npix * 16));

    // the level map: the passes fovpt_render ran for this frame
    const FrameDev& fd = c->rendered.frame;
    DenoiseArgs a;
    memset(&a, 0, sizeof(a));
    if (c->rendered.uniform) a.n_pass[0] = dc->iterations_uniform;
    else { a.n_pass[0] = dc->iterations_periphery; a.n_pass[1] = dc->iterations_middle; a.n_pass[2] = dc->iterations_fovea; }
    for (int p = 0; p < fd.npass; p++) a.iterations = a.n_pass[p] > a.iterations ? a.n_pass[p] : a.iterations;
    a.inv_c = inv_sq(dc->color_sigma); a.inv_n = inv_sq(dc->normal_sigma); a.inv_a = inv_sq(dc->albedo_sigma);
    fovpt_launch_denoise(c->shadow_stream, fd, a, lp->frame.color_buffer, lp->frame.normal_buffer, lp->frame.albedo_buffer,
                         (float4*)c->denoise.i0.p, (float4*)c->denoise.i1.p, (uint8_t*)c->denoise.level.p, out_color, out_rgba);
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

// fovpt_reconstruct's validation.  in: its colour input, or null where an earlier stage of fovpt_post makes it
int reconstruct_check(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_reconstruct_config* rc, const fovpt_float4* in, const char* who)
{
    if (!(rc->support >= 1.0f && rc->support <= 2.0f)) return fail(c, FOVPT_E_INVALID, "%s: support %g outside [1, 2]", who, (double)rc->support);
    const float sig[2] = {rc->normal_sigma, rc->depth_sigma};
    for (float v : sig)
        if (!sigma_ok(v)) return fail(c, FOVPT_E_INVALID, "%s: sigma %g outside [%g, %g]", who, (double)v, (double)FOVPT_SIGMA_MIN, (double)FOVPT_SIGMA_MAX);
    if (rc->levels < 0 || rc->levels > 3) return fail(c, FOVPT_E_INVALID, "%s: levels %d outside 0 .. 3", who, rc->levels);
    if (rc->remodulate != 0 && rc->remodulate != 1) return fail(c, FOVPT_E_INVALID, "%s: remodulate %d is neither 0 nor 1", who, rc->remodulate);
    CHK(check_reserved(c, rc->_reserved, sizeof(rc->_reserved) / 4, who));
    if (!c->has_scene || lp->traversable != c->scene_id) return fail(c, FOVPT_E_NO_SCENE, "%s without a scene", who);
    const char* need_guides = "fovpt_reconstruct with remodulate = 1 needs the albedo guide: the frame was rendered without fovpt_config.write_guides = 1 (not available with shadow-catcher materials)";
    CHK(check_rendered_frame(c, lp, who, "reconstruct from", rc->remodulate ? need_guides : nullptr, 0));
    if (!in) return fail(c, FOVPT_E_INVALID, "%s: null accum_buffer", who);
    if (rc->remodulate && !lp->frame.albedo_buffer) return fail(c, FOVPT_E_INVALID, "%s: null albedo guide", who);
    return FOVPT_OK;
}

ReconstructArgs reconstruct_args(const fovpt_reconstruct_config* rc)
{
    ReconstructArgs a;
    memset(&a, 0, sizeof(a));
    const float s = rc->support;
    a.inv_support[0] = 1.0f / (s * 2.0f);
    a.inv_support[1] = 1.0f / (s * 4.0f);
    a.inv_n = inv_sq(rc->normal_sigma); a.inv_z = inv_sq(rc->depth_sigma);
    a.levels = rc->levels; a.remodulate = rc->remodulate;
    return a;
}

// the rendered frame's G-buffer (into fovpt_gbuffer's buffers) and the reconstruction, for a checked call with its outputs set
int reconstruct_enqueue(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_reconstruct_config* rc, const fovpt_float4* in,
                        fovpt_float4* out_color, uint32_t* out_rgba, const char* who)
{
    GBufferDev g;
    CHK(enqueue_gbuffer(c, lp, c->rendered.frame, g, who));               // the rendered frame's camera
    fovpt_launch_reconstruct(c->shadow_stream, c->rendered.frame, reconstruct_args(rc), in, lp->frame.albedo_buffer, g, out_color, out_rgba);
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

// the validation of fovpt_temporal and fovpt_temporal_motion.  in: as reconstruct_check's
int temporal_check(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_temporal_config* tc, const fovpt_float4* in, const char* who)
{
    const int32_t caps[4] = {tc->history_fovea, tc->history_middle, tc->history_periphery, tc->history_uniform};
    for (int32_t v : caps)
        if (v < 1 || v > FOVPT_TEMPORAL_MAX_HISTORY) return fail(c, FOVPT_E_INVALID, "%s: history cap %d outside 1 .. %d", who, v, FOVPT_TEMPORAL_MAX_HISTORY);
    if (!(tc->normal_tolerance >= 0.0f && tc->normal_tolerance <= 4.0f))
        return fail(c, FOVPT_E_INVALID, "%s: normal_tolerance %g outside [0, 4]", who, (double)tc->normal_tolerance);
    if (!(tc->depth_tolerance >= 0.0f && tc->depth_tolerance <= 1.0f))
        return fail(c, FOVPT_E_INVALID, "%s: depth_tolerance %g outside [0, 1]", who, (double)tc->depth_tolerance);
    CHK(check_reserved(c, tc->_reserved, sizeof(tc->_reserved) / 4, who));
    if (!c->has_scene || lp->traversable != c->scene_id) return fail(c, FOVPT_E_NO_SCENE, "%s without a scene", who);
    CHK(check_rendered_frame(c, lp, who, "reproject from", nullptr, 0));
    if (!in) return fail(c, FOVPT_E_INVALID, "%s: null accum_buffer", who);
    return FOVPT_OK;
}

// what a temporal step's outputs must not be (the histories exist: reserve_temporal)
int temporal_alias_check(fovpt_ctx* c, const fovpt_float4* in, const fovpt_float4* out_color, const uint32_t* out_rgba, const fovpt_float4* out_motion,
                         const char* who)
{
    const void *h0 = c->temporal.hist[0].p, *h1 = c->temporal.hist[1].p;
    if ((void*)out_color == h0 || (void*)out_color == h1)
        return fail(c, FOVPT_E_INVALID, "%s: the output colour buffer is the context's history", who);
    if (out_motion && (out_motion == out_color || (void*)out_motion == (void*)out_rgba || out_motion == in || (void*)out_motion == h0 || (void*)out_motion == h1))
        return fail(c, FOVPT_E_INVALID, "%s: the motion buffer is another buffer of the call or the context's history", who);
    return FOVPT_OK;
}

// One step of the history, for a checked call with its outputs set: fovpt_temporal's (motion false: k_temporal, and no HIP call
// beside those of the G-buffer and that launch) or fovpt_temporal_motion's (motion true: k_temporal_motion; the first one of a
// scene switches the tracking of previous positions on).  Either ends the interval in which fovpt_update_vertices marks meshes
// as moved.  With `fuse` (fovpt_post) the step's input is the reconstruction of `in` by those arguments, made from the step's own
// G-buffer set inside the step's kernel (k_reconstruct_temporal) and written nowhere.
int temporal_enqueue(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_temporal_config* tc, const fovpt_float4* in,
                     fovpt_float4* out_color, uint32_t* out_rgba, fovpt_float4* out_motion, bool motion, const char* who,
                     const ReconstructArgs* fuse = nullptr)
{
    const hipStream_t st = c->shadow_stream;
    fovpt_ctx::Temporal& T = c->temporal;
    if (motion && !c->tm_tracking) {                                       // the marks: no mesh has moved yet (0 is no step's number)
        const size_t nmesh = c->mesh_nv.size();
        HIPCHK(c, c->tm_mark.reserve(nmesh * sizeof(uint64_t)));
        HIPCHK(c, hipMemsetAsync(c->tm_mark.p, 0, nmesh * sizeof(uint64_t), st));
        c->tm_mesh_epoch.assign(nmesh, 0ull);
        c->tm_tracking = true;
    }
    const int cur = T.last ^ 1, prev = T.last;
    const GBufferDev g = temporal_set(c, cur), gp = temporal_set(c, prev);
    GBufferDev gt;
    CHK(enqueue_gbuffer(c, lp, c->rendered.frame, gt, who, &g));          // the rendered frame's camera
    const FrameDev& fd = c->rendered.frame;
    TemporalArgs a;
    memset(&a, 0, sizeof(a));
    a.cap[0] = tc->history_fovea; a.cap[1] = tc->history_middle; a.cap[2] = tc->history_periphery; a.cap[3] = tc->history_uniform;
    a.normal_tol = tc->normal_tolerance; a.depth_tol = tc->depth_tolerance;
    a.uniform = c->rendered.uniform != 0;
    a.reproject = T.valid && T.w == c->rendered.w && T.h == c->rendered.h && camera_inverse(T.U, T.V, T.W, a.inv);
    memcpy(a.eye_prev, T.eye, sizeof(a.eye_prev));
    const float4* hist_prev = (const float4*)T.hist[prev].p;
    float4* hist_out = (float4*)T.hist[cur].p;
    TemporalMotionArgs m;
    memset(&m, 0, sizeof(m));
    if (motion) {
        if (c->tm_untracked) a.reproject = 0;                              // meshes moved unrecorded: where they were is not known
        m.hit = (const float4*)c->gbuffer.hit.p; m.tris = c->tris;
        m.mark = (const uint64_t*)c->tm_mark.p; m.epoch = c->tm_epoch;
        m.tri_vidx = (const uint3*)c->up_vidx.p; m.vtx_prev = (const float*)c->vtx_prev.p;
        m.out_motion = out_motion;
    }
    if (fuse) fovpt_launch_reconstruct_temporal(st, fd, *fuse, a, motion ? &m : nullptr, in, lp->frame.albedo_buffer, g, gp, hist_prev, hist_out, out_color, out_rgba);
    else if (!motion) fovpt_launch_temporal(st, fd, a, in, g, gp, hist_prev, hist_out, out_color, out_rgba);
    else fovpt_launch_temporal_motion(st, fd, a, m, in, g, gp, hist_prev, hist_out, out_color, out_rgba);
    HIPCHK(c, hipGetLastError());
    T.last = cur;                                                          // this step is the next one's previous step
    T.valid = true;
    T.w = c->rendered.w; T.h = c->rendered.h;
    memcpy(T.eye, fd.eye, sizeof(T.eye)); memcpy(T.U, fd.U, sizeof(T.U));
    memcpy(T.V, fd.V, sizeof(T.V)); memcpy(T.W, fd.W, sizeof(T.W));
    c->tm_epoch++;                                                         // the marks of this interval no longer hold
    c->tm_step_blind = c->tm_untracked;                                    // fovpt_warp_motion: what this step knew of the interval it ended
    c->seq_step = ++c->seq;
    c->tm_untracked = false;
    return FOVPT_OK;
}

// fovpt_temporal (motion false) and fovpt_temporal_motion (motion true)
int temporal_step(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_temporal_config* tc, const fovpt_float4* in_color,
                  fovpt_float4* out_color, uint32_t* out_rgba, fovpt_float4* out_motion, bool motion, const char* who)
{
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !tc) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    const fovpt_float4* in = in_color ? in_color : lp->frame.accum_buffer;
    CHK(temporal_check(c, lp, tc, in, who));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(reserve_temporal(c, c->rendered.pixels()));
    CHK(own_outputs(c, who, c->temporal.out, out_color, out_rgba));
    CHK(temporal_alias_check(c, in, out_color, out_rgba, out_motion, who));
    return temporal_enqueue(c, lp, tc, in, out_color, out_rgba, out_motion, motion, who);
}

// what fovpt_variance and fovpt_variance_filter ask of the scene, the rendered frame and a caller's G-buffer (need_albedo: the
// filter demodulates), after their configs are checked.  in: the colour input
int variance_frame_check(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_gbuffer_ptrs* gbuffer, bool need_albedo, const fovpt_float4* in,
                         const char* who, const char* to_what)
{
    if (!gbuffer && (!c->has_scene || lp->traversable != c->scene_id)) return fail(c, FOVPT_E_NO_SCENE, "%s without a scene", who);
#if FOVPT_V_STEPSTAT
    if (!gbuffer) return fail(c, FOVPT_E_INVALID, "%s: the G-buffer is not available in a diagnostic (FOVPT_V_STEPSTAT) build", who);
#endif
    CHK(check_rendered_frame(c, lp, who, to_what, nullptr, 1ull << 31));
    if (gbuffer && (gbuffer->width != c->rendered.w || gbuffer->height != c->rendered.h || !gbuffer->position || !gbuffer->normal))
        return fail(c, FOVPT_E_INVALID, "%s: the G-buffer is not of the frame's size %d x %d, or has a null position or normal", who, c->rendered.w, c->rendered.h);
    if (gbuffer && need_albedo && !gbuffer->albedo) return fail(c, FOVPT_E_INVALID, "%s: demodulate = 1 with a G-buffer that has a null albedo", who);
    if (!in) return fail(c, FOVPT_E_INVALID, "%s: null accum_buffer", who);
    return FOVPT_OK;
}

// fovpt_variance's validation; makes the kernel's arguments but has_history
int variance_check(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_variance_config* vc, const fovpt_gbuffer_ptrs* gbuffer, const fovpt_float4* in,
                   const char* who, VarianceArgs& a)
{
    if (vc->history_cap < 1 || vc->history_cap > FOVPT_TEMPORAL_MAX_HISTORY)
        return fail(c, FOVPT_E_INVALID, "%s: history_cap %d outside 1 .. %d", who, vc->history_cap, FOVPT_TEMPORAL_MAX_HISTORY);
    if (vc->spatial_below < 0 || vc->spatial_below > vc->history_cap + 1)
        return fail(c, FOVPT_E_INVALID, "%s: spatial_below %d outside 0 .. history_cap + 1", who, vc->spatial_below);
    if (vc->spatial_radius < 1 || vc->spatial_radius > 3) return fail(c, FOVPT_E_INVALID, "%s: spatial_radius %d outside 1 .. 3", who, vc->spatial_radius);
    if (!(vc->depth_tolerance >= 0.0f && vc->depth_tolerance <= 1.0f))
        return fail(c, FOVPT_E_INVALID, "%s: depth_tolerance %g outside [0, 1]", who, (double)vc->depth_tolerance);
    if (!(vc->normal_tolerance >= 0.0f && vc->normal_tolerance <= 4.0f))
        return fail(c, FOVPT_E_INVALID, "%s: normal_tolerance %g outside [0, 4]", who, (double)vc->normal_tolerance);
    CHK(check_reserved(c, vc->_reserved, sizeof(vc->_reserved) / 4, who));
    CHK(variance_frame_check(c, lp, gbuffer, false, in, who, "estimate variance from"));
    const FrameDev& fd = c->rendered.frame;
    float M[9];
    if (!camera_inverse(fd.U, fd.V, fd.W, M)) return fail(c, FOVPT_E_INVALID, "%s: the rendered camera is singular", who);
    memset(&a, 0, sizeof(a));
    memcpy(a.eye, fd.eye, sizeof(a.eye)); memcpy(a.m2, M + 6, sizeof(a.m2));
    a.depth_tol = vc->depth_tolerance; a.normal_tol = vc->normal_tolerance;
    a.cap = vc->history_cap; a.spatial_below = vc->spatial_below; a.radius = vc->spatial_radius;
    return FOVPT_OK;
}

// fovpt_variance_filter's validation.  variance: the caller's, or null for the context's own image
int variance_filter_check(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_variance_filter_config* fc, const fovpt_gbuffer_ptrs* gbuffer,
                          const fovpt_float4* in, const fovpt_float4* variance, const char* who)
{
    const int32_t its[4] = {fc->iterations_fovea, fc->iterations_middle, fc->iterations_periphery, fc->iterations_uniform};
    for (int32_t n : its)
        if (n < 0 || n > FOVPT_DENOISE_MAX_ITERATIONS) return fail(c, FOVPT_E_INVALID, "%s: iteration count %d outside 0 .. %d", who, n, FOVPT_DENOISE_MAX_ITERATIONS);
    const float sig[3] = {fc->luminance_sigma, fc->normal_sigma, fc->depth_sigma};
    for (float v : sig)
        if (!sigma_ok(v)) return fail(c, FOVPT_E_INVALID, "%s: sigma %g outside [%g, %g]", who, (double)v, (double)FOVPT_SIGMA_MIN, (double)FOVPT_SIGMA_MAX);
    if (fc->demodulate != 0 && fc->demodulate != 1) return fail(c, FOVPT_E_INVALID, "%s: demodulate %d is neither 0 nor 1", who, fc->demodulate);
    CHK(check_reserved(c, fc->_reserved, sizeof(fc->_reserved) / 4, who));
    CHK(variance_frame_check(c, lp, gbuffer, fc->demodulate != 0, in, who, "filter with"));
    if (!variance && (c->variance.own_w != c->rendered.w || c->variance.own_h != c->rendered.h))
        return fail(c, FOVPT_E_NO_FRAME, "%s: no fovpt_variance has written the context's variance image at this frame size", who);
    return FOVPT_OK;
}

// fovpt_bloom's validation.  in: its colour input
int bloom_check(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_bloom_config* bc, const fovpt_float4* in, const char* who)
{
    if (bc->flags & ~(FOVPT_BLOOM_KARIS | FOVPT_BLOOM_GAINS | FOVPT_BLOOM_EXPOSURE_STATE)) return fail(c, FOVPT_E_INVALID, "%s: unknown flag bits in %d", who, bc->flags);
    if (bc->levels < 1 || bc->levels > FOVPT_BLOOM_MAX_LEVELS) return fail(c, FOVPT_E_INVALID, "%s: levels %d outside 1 .. %d", who, bc->levels, FOVPT_BLOOM_MAX_LEVELS);
    const float pos[2] = {bc->threshold, bc->exposure};
    for (float v : pos)
        if (!sigma_ok(v)) return fail(c, FOVPT_E_INVALID, "%s: threshold or exposure %g outside [%g, %g]", who, (double)v, (double)FOVPT_SIGMA_MIN, (double)FOVPT_SIGMA_MAX);
    const float nonneg[2] = {bc->knee, bc->intensity};
    for (float v : nonneg)
        if (!(v >= 0.0f && v <= FOVPT_SIGMA_MAX)) return fail(c, FOVPT_E_INVALID, "%s: knee or intensity %g outside [0, %g]", who, (double)v, (double)FOVPT_SIGMA_MAX);
    const float unit[5] = {bc->spread, bc->gain_fovea, bc->gain_middle, bc->gain_periphery, bc->gain_uniform};
    for (float v : unit)
        if (!(v >= 0.0f && v <= 1.0f)) return fail(c, FOVPT_E_INVALID, "%s: spread or gain %g outside [0, 1]", who, (double)v);
    CHK(check_reserved(c, bc->_reserved, sizeof(bc->_reserved) / 4, who));
    CHK(check_rendered_frame(c, lp, who, "spread light over", nullptr, 1ull << 31));
    if (!in) return fail(c, FOVPT_E_INVALID, "%s: null accum_buffer", who);
    return FOVPT_OK;
}

BloomArgs bloom_args(const fovpt_bloom_config* bc, const fovpt_ctx::Rendered& R)
{
    BloomArgs a;
    memset(&a, 0, sizeof(a));
    a.flags = bc->flags; a.uniform = R.uniform != 0;
    a.threshold = bc->threshold; a.knee = bc->knee; a.exposure = bc->exposure; a.intensity = bc->intensity; a.spread = bc->spread;
    a.gain[0] = bc->gain_fovea; a.gain[1] = bc->gain_middle; a.gain[2] = bc->gain_periphery; a.gain[3] = bc->gain_uniform;
    return a;
}

// the launches of a checked call with its outputs set and the pyramid reserved
int bloom_enqueue(fovpt_ctx* c, const fovpt_bloom_config* bc, const fovpt_float4* in, fovpt_float4* out_color, uint32_t* out_rgba)
{
    const fovpt_ctx::Rendered& R = c->rendered;
    // the exposure record where fovpt_expose has made one (none yet: no AUTO step has run, E = cfg.exposure)
    const ExposeState* state = (bc->flags & FOVPT_BLOOM_EXPOSURE_STATE) ? (const ExposeState*)c->expose.state.p : nullptr;
    fovpt_launch_bloom(c->shadow_stream, R.frame, bloom_args(bc, R), bc->levels, state, in, (float4*)c->bloom.pyramid.p, out_color, out_rgba);
    HIPCHK(c, hipGetLastError());
    int W, H;
    fovpt_bloom_level(R.w, R.h, bc->levels, &W, &H, &c->bloom.texels);
    return FOVPT_OK;
}

}  // namespace

// fovpt_reconstruct_defaults (chosen by measurement: DESIGN.md, section 11)
#define FOVPT_RECONSTRUCT_SUPPORT 2.0f
#define FOVPT_RECONSTRUCT_NORMAL_SIGMA 0.5f
#define FOVPT_RECONSTRUCT_DEPTH_SIGMA 0.05f

// fovpt_temporal_defaults (chosen by measurement: DESIGN.md, section 12)
#define FOVPT_TEMPORAL_HISTORY_FOVEA 1
#define FOVPT_TEMPORAL_HISTORY_MIDDLE 4
#define FOVPT_TEMPORAL_HISTORY_PERIPHERY 8
#define FOVPT_TEMPORAL_HISTORY_UNIFORM 4
#define FOVPT_TEMPORAL_NORMAL_TOLERANCE 0.1f
#define FOVPT_TEMPORAL_DEPTH_TOLERANCE 0.02f

// edge-stopping scales of fovpt_denoise_defaults (chosen by measurement: DESIGN.md, denoiser)
#define FOVPT_DENOISE_COLOR_SIGMA 8.0f
#define FOVPT_DENOISE_NORMAL_SIGMA 0.5f
#define FOVPT_DENOISE_ALBEDO_SIGMA 0.2f

extern "C" {

// ---- denoiser of the rendered frame (denoise.hip; the filter's definition: tests/denoise_ref.py) ------------------------
int fovpt_denoise_defaults(fovpt_denoise_config* out)
{
    if (!zeroed(out)) return FOVPT_E_INVALID;
    out->iterations_fovea = 0;
    out->iterations_middle = 2;
    out->iterations_periphery = 3;
    out->iterations_uniform = 3;
    out->color_sigma = FOVPT_DENOISE_COLOR_SIGMA;
    out->normal_sigma = FOVPT_DENOISE_NORMAL_SIGMA;
    out->albedo_sigma = FOVPT_DENOISE_ALBEDO_SIGMA;
    return FOVPT_OK;
}

int fovpt_denoise_buffers(fovpt_ctx* c, fovpt_float4** color, uint32_t** rgba)
{
    return c ? own_buffers(c, "fovpt_denoise_buffers", c->denoise.out, color, rgba) : FOVPT_E_INVALID;
}

// Enqueued on the stream every resolve runs on (fovpt_stream()), in issue order: behind the resolve of the frame last issued
// -- also with frames_in_flight = 2 or chains_per_frame = 2, whose chains all join that stream for their resolve -- and ahead
// of the next frame's resolve, the first of its launches that rewrites accum / frame / guides (its memsets and snapshot copies
// of chunked launches also run there).  Callers synchronising on fovpt_stream() see the denoised frame.
int fovpt_denoise(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_denoise_config* dc, fovpt_float4* out_color, uint32_t* out_rgba)
{
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !dc) return fail(c, FOVPT_E_INVALID, "fovpt_denoise: null argument");
    CHK(denoise_check(c, lp, dc, "fovpt_denoise"));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(own_outputs(c, "fovpt_denoise", c->denoise.out, out_color, out_rgba));
    return denoise_enqueue(c, lp, dc, out_color, out_rgba);
}

// ---- G-buffer and reconstruction of the rendered frame (reconstruct.hip; the reconstruction's definition:
// tests/reconstruct_ref.py) --------------------------------------------------------------------------------------------
int fovpt_gbuffer(fovpt_ctx* c, const fovpt_launch_params* lp, fovpt_gbuffer_ptrs* out)
{
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !out) return fail(c, FOVPT_E_INVALID, "fovpt_gbuffer: null argument");
    GBufferDev g;
    FrameDev view;
    memset(&view, 0, sizeof(view));
    set_camera(view, lp);
    CHK(enqueue_gbuffer(c, lp, view, g, "fovpt_gbuffer"));
    gbuffer_ptrs(g, lp->frame.size.x, lp->frame.size.y, out);
    return FOVPT_OK;
}

int fovpt_reconstruct_defaults(fovpt_reconstruct_config* out)
{
    if (!zeroed(out)) return FOVPT_E_INVALID;
    out->support = FOVPT_RECONSTRUCT_SUPPORT;
    out->normal_sigma = FOVPT_RECONSTRUCT_NORMAL_SIGMA;
    out->depth_sigma = FOVPT_RECONSTRUCT_DEPTH_SIGMA;
    out->levels = 3;
    out->remodulate = 1;
    return FOVPT_OK;
}

int fovpt_reconstruct_buffers(fovpt_ctx* c, fovpt_float4** color, uint32_t** rgba)
{
    return c ? own_buffers(c, "fovpt_reconstruct_buffers", c->reconstruct.out, color, rgba) : FOVPT_E_INVALID;
}

// Enqueued on fovpt_stream() like fovpt_denoise, and ordered like it: behind the resolve of the frame last issued, ahead of
// the next frame's.  Builds that frame's G-buffer first (the same stream), then reconstructs.
int fovpt_reconstruct(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_reconstruct_config* rc, const fovpt_float4* in_color,
                      fovpt_float4* out_color, uint32_t* out_rgba)
{
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !rc) return fail(c, FOVPT_E_INVALID, "fovpt_reconstruct: null argument");
    const fovpt_float4* in = in_color ? in_color : lp->frame.accum_buffer;
    CHK(reconstruct_check(c, lp, rc, in, "fovpt_reconstruct"));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(own_outputs(c, "fovpt_reconstruct", c->reconstruct.out, out_color, out_rgba));
    if (in == out_color) return fail(c, FOVPT_E_INVALID, "fovpt_reconstruct: the input is the output colour buffer (it reads neighbours)");
    return reconstruct_enqueue(c, lp, rc, in, out_color, out_rgba, "fovpt_reconstruct");
}

// ---- temporal reprojection of the frame history (temporal.hip; its definition: tests/temporal_ref.py) ------------------
int fovpt_temporal_defaults(fovpt_temporal_config* out)
{
    if (!zeroed(out)) return FOVPT_E_INVALID;
    out->history_fovea = FOVPT_TEMPORAL_HISTORY_FOVEA;
    out->history_middle = FOVPT_TEMPORAL_HISTORY_MIDDLE;
    out->history_periphery = FOVPT_TEMPORAL_HISTORY_PERIPHERY;
    out->history_uniform = FOVPT_TEMPORAL_HISTORY_UNIFORM;
    out->normal_tolerance = FOVPT_TEMPORAL_NORMAL_TOLERANCE;
    out->depth_tolerance = FOVPT_TEMPORAL_DEPTH_TOLERANCE;
    return FOVPT_OK;
}

int fovpt_temporal_buffers(fovpt_ctx* c, fovpt_float4** color, uint32_t** rgba, const fovpt_float4** history)
{
    if (!c || !history) return FOVPT_E_INVALID;
    CHK(own_buffers(c, "fovpt_temporal_buffers", c->temporal.out, color, rgba));
    if (!c->temporal.hist[0].p) CHK(reserve_temporal(c, c->rendered.pixels()));      // the histories and G-buffer sets with them
    *history = (const fovpt_float4*)c->temporal.hist[c->temporal.last].p;
    return FOVPT_OK;
}

int fovpt_temporal_reset(fovpt_ctx* c)
{
    if (!c) return FOVPT_E_INVALID;
    c->temporal.valid = false;
    return FOVPT_OK;
}

int fovpt_temporal_gbuffer(fovpt_ctx* c, fovpt_gbuffer_ptrs* out)
{
    if (!c) return FOVPT_E_INVALID;
    if (!out) return fail(c, FOVPT_E_INVALID, "fovpt_temporal_gbuffer: null argument");
    if (!c->temporal.valid) return fail(c, FOVPT_E_NO_FRAME, "fovpt_temporal_gbuffer: no temporal step since create / reset / resize / set_scene");
    gbuffer_ptrs(temporal_set(c, c->temporal.last), c->temporal.w, c->temporal.h, out);
    return FOVPT_OK;
}

// Enqueued on fovpt_stream() like fovpt_reconstruct, and ordered like it.  Traces the rendered frame's G-buffer into the set
// the last call did not write, reprojects the other set's history into it, and makes it the last written.
int fovpt_temporal(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_temporal_config* tc, const fovpt_float4* in_color,
                   fovpt_float4* out_color, uint32_t* out_rgba)
{
    return temporal_step(c, lp, tc, in_color, out_color, out_rgba, nullptr, false, "fovpt_temporal");
}

// fovpt_temporal with moved meshes reprojected by their own motion (k_temporal_motion) and, with out_motion, motion vectors.
int fovpt_temporal_motion(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_temporal_config* tc, const fovpt_float4* in_color,
                          fovpt_float4* out_color, uint32_t* out_rgba, fovpt_float4* out_motion)
{
    return temporal_step(c, lp, tc, in_color, out_color, out_rgba, out_motion, true, "fovpt_temporal_motion");
}

// ---- the post-frame chain in one call (the fused kernel: post_fused.hip; its definition: tests/post_ref.py) --------------
int fovpt_post_defaults(fovpt_post_config* out)
{
    if (!zeroed(out)) return FOVPT_E_INVALID;
    out->stages = FOVPT_POST_RECONSTRUCT | FOVPT_POST_TEMPORAL | FOVPT_POST_MOTION;
    (void)fovpt_denoise_defaults(&out->denoise);
    (void)fovpt_reconstruct_defaults(&out->reconstruct);
    (void)fovpt_temporal_defaults(&out->temporal);
    return FOVPT_OK;
}

int fovpt_post_buffers(fovpt_ctx* c, fovpt_float4** color, uint32_t** rgba)
{
    return c ? own_buffers(c, "fovpt_post_buffers", c->post.out, color, rgba) : FOVPT_E_INVALID;
}

// The enabled stage calls one after the other, on fovpt_stream() and ordered like them -- except that the reconstruction and the
// temporal step together are one G-buffer trace (into the step's set) and one kernel.  Every stage is checked before the first
// is enqueued and before any state of the step moves.
int fovpt_post(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_post_config* pc, const fovpt_float4* in_color, fovpt_float4* out_color,
               uint32_t* out_rgba, fovpt_float4* out_motion)
{
    const char* who = "fovpt_post";
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !pc) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    const int32_t all = FOVPT_POST_DENOISE | FOVPT_POST_RECONSTRUCT | FOVPT_POST_TEMPORAL | FOVPT_POST_MOTION;
    if (pc->stages == 0 || (pc->stages & ~all)) return fail(c, FOVPT_E_INVALID, "%s: stages %d names no stage or an unknown one", who, pc->stages);
    const bool D = pc->stages & FOVPT_POST_DENOISE, R = pc->stages & FOVPT_POST_RECONSTRUCT, T = pc->stages & FOVPT_POST_TEMPORAL,
               M = pc->stages & FOVPT_POST_MOTION;
    if (M && !T) return fail(c, FOVPT_E_INVALID, "%s: FOVPT_POST_MOTION needs FOVPT_POST_TEMPORAL", who);
    if (out_motion && !M) return fail(c, FOVPT_E_INVALID, "%s: a motion buffer without FOVPT_POST_MOTION", who);
    if (in_color && D) return fail(c, FOVPT_E_INVALID, "%s: in_color with FOVPT_POST_DENOISE (the denoiser reads the frame's accum and guides)", who);
    CHK(check_reserved(c, pc->_reserved, sizeof(pc->_reserved) / 4, who));
#if FOVPT_V_STEPSTAT
    if (R || T) return fail(c, FOVPT_E_INVALID, "%s: the G-buffer is not available in a diagnostic (FOVPT_V_STEPSTAT) build", who);
#endif
    // the later stages' colour input where no stage makes it (a stage's output is never null: any non-null value stands for it)
    const fovpt_float4* in0 = in_color ? in_color : lp->frame.accum_buffer;
    const fovpt_float4* const made = (const fovpt_float4*)c;
    if (D) CHK(denoise_check(c, lp, &pc->denoise, who));
    if (R) CHK(reconstruct_check(c, lp, &pc->reconstruct, D ? made : in0, who));
    if (T) CHK(temporal_check(c, lp, &pc->temporal, D || R ? made : in0, who));

    // buffers: the denoiser's own where a stage follows it, the step's sets and histories, the call's outputs
    HIPCHK(c, hipSetDevice(c->device));
    fovpt_float4* dn_color = nullptr;
    uint32_t* dn_rgba = nullptr;
    if (D && (R || T)) CHK(own_outputs(c, who, c->denoise.out, dn_color, dn_rgba));
    if (T) CHK(reserve_temporal(c, c->rendered.pixels()));
    CHK(own_outputs(c, who, c->post.out, out_color, out_rgba));
    const fovpt_float4* in = D ? dn_color : in0;                            // what the stage after the denoiser reads
    if (R && in == out_color) return fail(c, FOVPT_E_INVALID, "%s: the reconstruction's input is the output colour buffer (it reads neighbours)", who);
    if (T) CHK(temporal_alias_check(c, in, out_color, out_rgba, out_motion, who));
    if (R && T) {                                                          // one kernel reads `in` and the albedo guide across pixels
        const void* wr[4] = {out_rgba, out_motion, c->temporal.hist[0].p, c->temporal.hist[1].p};
        const void* alb = pc->reconstruct.remodulate ? (const void*)lp->frame.albedo_buffer : nullptr;
        for (const void* w : wr)
            if (w && (w == (const void*)in || w == alb)) return fail(c, FOVPT_E_INVALID, "%s: an output or history buffer is the reconstruction's input or the albedo guide", who);
        if (alb && (const void*)out_color == alb) return fail(c, FOVPT_E_INVALID, "%s: the output colour buffer is the albedo guide", who);
    }

    if (D) CHK(R || T ? denoise_enqueue(c, lp, &pc->denoise, dn_color, dn_rgba) : denoise_enqueue(c, lp, &pc->denoise, out_color, out_rgba));
    if (R && !T) return reconstruct_enqueue(c, lp, &pc->reconstruct, in, out_color, out_rgba, who);
    if (T) {
        ReconstructArgs ra;
        if (R) ra = reconstruct_args(&pc->reconstruct);
        return temporal_enqueue(c, lp, &pc->temporal, in, out_color, out_rgba, out_motion, M, who, R ? &ra : nullptr);
    }
    return FOVPT_OK;
}

// ---- luminance moment history and variance-guided a-trous filter (variance.hip; their definition: tests/variance_ref.py) ----------
// (conventions, not measurements: SVGF's history, threshold and window, fovpt_temporal's tolerances)
int fovpt_variance_defaults(fovpt_variance_config* out)
{
    if (!zeroed(out)) return FOVPT_E_INVALID;
    out->history_cap = 16;
    out->spatial_below = 4;
    out->spatial_radius = 3;
    out->depth_tolerance = FOVPT_TEMPORAL_DEPTH_TOLERANCE;
    out->normal_tolerance = FOVPT_TEMPORAL_NORMAL_TOLERANCE;
    return FOVPT_OK;
}

int fovpt_variance_buffers(fovpt_ctx* c, fovpt_float4** variance, const fovpt_float4** moments)
{
    if (!c || !variance || !moments) return FOVPT_E_INVALID;
    *variance = nullptr; *moments = nullptr;
    fovpt_ctx::Variance& V = c->variance;
    if (!V.image.p) {
        if (c->rendered.w <= 0 || c->rendered.h <= 0) return fail(c, FOVPT_E_NO_FRAME, "fovpt_variance_buffers: no frame rendered yet");
        HIPCHK(c, hipSetDevice(c->device));
    }
    CHK(reserve_variance(c, c->rendered.pixels()));
    *variance = (fovpt_float4*)V.image.p;
    *moments = (const fovpt_float4*)V.hist[V.last].p;
    return FOVPT_OK;
}

int fovpt_variance_reset(fovpt_ctx* c)
{
    if (!c) return FOVPT_E_INVALID;
    c->variance.valid = false;
    return FOVPT_OK;
}

// Enqueued on fovpt_stream() like fovpt_denoise, and ordered like it.  Without a caller's G-buffer the rendered frame's first (the same
// stream, into fovpt_gbuffer's buffers); then one launch of k_variance_moments, from the history the last call wrote into the other.
int fovpt_variance(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_variance_config* vc, const fovpt_gbuffer_ptrs* gbuffer,
                   const fovpt_float4* in_sample, const fovpt_float4* motion, fovpt_float4* out_variance)
{
    const char* who = "fovpt_variance";
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !vc) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    const fovpt_float4* in = in_sample ? in_sample : lp->frame.accum_buffer;
    VarianceArgs a;
    CHK(variance_check(c, lp, vc, gbuffer, in, who, a));
    HIPCHK(c, hipSetDevice(c->device));
    fovpt_ctx::Variance& V = c->variance;
    const fovpt_ctx::Rendered& R = c->rendered;
    CHK(reserve_variance(c, R.pixels()));
    const bool own = !out_variance;
    if (own) out_variance = (fovpt_float4*)V.image.p;
    GBufferDev g = gbuffer_dev(c, gbuffer);                                // (the context's own: null until the first trace)
    CHK(check_aliases(c, {out_variance}, {in, g.pos, g.nrm, motion, V.hist[0].p, V.hist[1].p}, who,
                      "%s: the output is an input of the call or a moment history (the kernel reads across pixels)"));
    if (!gbuffer) CHK(enqueue_gbuffer(c, lp, R.frame, g, who));           // the rendered frame's camera
    const int cur = V.last ^ 1, prev = V.last;
    a.has_history = V.valid && V.w == R.w && V.h == R.h;
    fovpt_launch_variance(c->shadow_stream, R.frame, a, in, g.pos, g.nrm, motion, (const float4*)V.hist[prev].p, (float4*)V.hist[cur].p, out_variance);
    HIPCHK(c, hipGetLastError());
    V.last = cur;                                                          // this step is the next one's previous step
    V.valid = true;
    V.w = R.w; V.h = R.h;
    if (own) { V.own_w = R.w; V.own_h = R.h; }
    return FOVPT_OK;
}

// (conventions, not measurements: SVGF's luminance scale, fovpt_reconstruct's normal and depth scales)
int fovpt_variance_filter_defaults(fovpt_variance_filter_config* out)
{
    if (!zeroed(out)) return FOVPT_E_INVALID;
    out->iterations_fovea = 0;
    out->iterations_middle = 2;
    out->iterations_periphery = 4;
    out->iterations_uniform = 4;
    out->luminance_sigma = 4.0f;
    out->normal_sigma = FOVPT_RECONSTRUCT_NORMAL_SIGMA;
    out->depth_sigma = FOVPT_RECONSTRUCT_DEPTH_SIGMA;
    out->demodulate = 1;
    return FOVPT_OK;
}

int fovpt_variance_filter_buffers(fovpt_ctx* c, fovpt_float4** color, uint32_t** rgba)
{
    return c ? own_buffers(c, "fovpt_variance_filter_buffers", c->variance.out, color, rgba) : FOVPT_E_INVALID;
}

// Enqueued on fovpt_stream() like fovpt_denoise, and ordered like it.  Without a caller's G-buffer the rendered frame's first; then
// k_vfilter_prep and one k_vfilter_step per iteration.
int fovpt_variance_filter(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_variance_filter_config* fc, const fovpt_gbuffer_ptrs* gbuffer,
                          const fovpt_float4* in_color, const fovpt_float4* variance, fovpt_float4* out_color, uint32_t* out_rgba)
{
    const char* who = "fovpt_variance_filter";
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !fc) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    const fovpt_float4* in = in_color ? in_color : lp->frame.accum_buffer;
    CHK(variance_filter_check(c, lp, fc, gbuffer, in, variance, who));
    HIPCHK(c, hipSetDevice(c->device));
    fovpt_ctx::Variance& V = c->variance;
    const fovpt_ctx::Rendered& R = c->rendered;
    CHK(own_outputs(c, who, V.out, out_color, out_rgba));
    if (!variance) variance = (const fovpt_float4*)V.image.p;
    GBufferDev g = gbuffer_dev(c, gbuffer);                                // (the context's own: null until the first trace)
    CHK(check_aliases(c, {out_color, out_rgba}, {in, variance, g.pos, g.nrm, fc->demodulate ? g.alb : nullptr}, who,
                      "%s: an output is an input of the call (the kernels gather across pixels)"));
    const size_t npix = R.pixels();
    HIPCHK(c, V.level.reserve(npix));
    HIPCHK(c, V.j0.reserve(npix * 16));
    HIPCHK(c, V.j1.reserve(npix * 16));
    if (!gbuffer) CHK(enqueue_gbuffer(c, lp, R.frame, g, who));           // the rendered frame's camera
    VFilterArgs a;
    memset(&a, 0, sizeof(a));
    if (R.uniform) a.n_pass[0] = fc->iterations_uniform;
    else { a.n_pass[0] = fc->iterations_periphery; a.n_pass[1] = fc->iterations_middle; a.n_pass[2] = fc->iterations_fovea; }
    for (int p = 0; p < R.frame.npass; p++) a.iterations = a.n_pass[p] > a.iterations ? a.n_pass[p] : a.iterations;
    a.demodulate = fc->demodulate;
    a.sl2 = fc->luminance_sigma * fc->luminance_sigma; a.inv_n = inv_sq(fc->normal_sigma); a.inv_z = inv_sq(fc->depth_sigma);
    fovpt_launch_vfilter(c->shadow_stream, R.frame, a, in, variance, g, (float4*)V.j0.p, (float4*)V.j1.p, (uint8_t*)V.level.p, out_color, out_rgba);
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

// ---- HDR glare ahead of the tone map (bloom.hip; its definition: tests/bloom_ref.py) ----------------------------------------
// (conventions, not measurements: the usual threshold, knee and levels of a dual-filter bloom, the shipped app's exposure)
int fovpt_bloom_defaults(fovpt_bloom_config* out)
{
    if (!zeroed(out)) return FOVPT_E_INVALID;
    out->flags = FOVPT_BLOOM_KARIS;
    out->levels = 6;
    out->threshold = 1.0f;
    out->knee = 0.5f;
    out->exposure = 16.0f;
    out->intensity = 0.05f;
    out->spread = 0.7f;
    out->gain_fovea = out->gain_middle = out->gain_periphery = out->gain_uniform = 1.0f;
    return FOVPT_OK;
}

int fovpt_bloom_buffers(fovpt_ctx* c, fovpt_float4** color, uint32_t** rgba)
{
    return c ? own_buffers(c, "fovpt_bloom_buffers", c->bloom.out, color, rgba) : FOVPT_E_INVALID;
}

// Enqueued on fovpt_stream() like fovpt_denoise, and ordered like it: k_bloom_prefilter, the levels down and back up (one launch
// each), k_bloom_composite.  With EXPOSURE_STATE the exposure goes from fovpt_expose's record into the first kernel, never through
// the host.
int fovpt_bloom(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_bloom_config* bc, const fovpt_float4* in_color, fovpt_float4* out_color,
                uint32_t* out_rgba)
{
    const char* who = "fovpt_bloom";
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !bc) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    const fovpt_float4* in = in_color ? in_color : lp->frame.accum_buffer;
    CHK(bloom_check(c, lp, bc, in, who));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(own_outputs(c, who, c->bloom.out, out_color, out_rgba));
    HIPCHK(c, c->bloom.pyramid.reserve(bloom_pyramid_texels(c->rendered.w, c->rendered.h) * 16));
    const void* pyr = c->bloom.pyramid.p;
    CHK(check_aliases(c, {out_color, out_rgba}, {pyr}, who, "%s: an output is the pyramid"));
    CHK(check_aliases(c, {out_rgba, pyr}, {in}, who, "%s: the rgba output or the pyramid is the input (only out_color may be)"));
    return bloom_enqueue(c, bc, in, out_color, out_rgba);
}

}  // extern "C"
