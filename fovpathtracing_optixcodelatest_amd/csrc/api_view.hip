// api_view.hip -- post-processing of the rendered frame over the C ABI, second half: the stages that take the finished image to the
// viewer -- fovpt_expose (expose.hip), fovpt_warp / fovpt_warp_motion (warp.hip), fovpt_focus (focus.hip), fovpt_lens (lens.hip) --
// and fovpt_quality (quality.hip), with their defaults.  The stages have the shape of those in api_post.hip, whose shared steps they
// use (fovpt_ctx.h): *_check (nothing allocated, enqueued or changed), *_args (the kernel's arguments from the config and the
// rendered frame's record; where a camera may have none, the check makes them) and *_enqueue (reservations and launches of a
// checked call); an entry point is null checks, check, hipSetDevice, own outputs, alias check, enqueue.  What an alias check
// needs of the context's buffers is reserved ahead of it (warp's keys, focus's pairs).  The lens is one launch: its entry point has it.
#include <cmath>
#include <cstring>

#include "fovpt_ctx.h"

namespace {

// ---- fovpt_expose ----------------------------------------------------------------------------------------------------------------
// in: its colour input
int expose_check(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_expose_config* ec, const fovpt_float4* in, const char* who)
{
    if (ec->mode != FOVPT_EXPOSE_FIXED && ec->mode != FOVPT_EXPOSE_AUTO) return fail(c, FOVPT_E_INVALID, "%s: unknown mode %d", who, ec->mode);
    if (ec->metering != FOVPT_METER_FRAME && ec->metering != FOVPT_METER_GAZE) return fail(c, FOVPT_E_INVALID, "%s: unknown metering %d", who, ec->metering);
    if (ec->tone != FOVPT_TONE_REINHARD && ec->tone != FOVPT_TONE_ACES) return fail(c, FOVPT_E_INVALID, "%s: unknown tone map %d", who, ec->tone);
    const int32_t wts[4] = {ec->weight_fovea, ec->weight_middle, ec->weight_periphery, ec->weight_uniform};
    for (int32_t v : wts)
        if (v < 0 || v > 255) return fail(c, FOVPT_E_INVALID, "%s: weight %d outside 0 .. 255", who, v);
    if (!(0 <= ec->low_permille && ec->low_permille < ec->high_permille && ec->high_permille <= 1000))
        return fail(c, FOVPT_E_INVALID, "%s: permille %d .. %d is not 0 <= low < high <= 1000", who, ec->low_permille, ec->high_permille);
    if (!(ec->ev_min >= -16.0f && ec->ev_min <= ec->ev_max && ec->ev_max <= 16.0f))
        return fail(c, FOVPT_E_INVALID, "%s: ev range %g .. %g is not -16 <= ev_min <= ev_max <= 16", who, (double)ec->ev_min, (double)ec->ev_max);
    const float pos[3] = {ec->key, ec->exposure, ec->white};
    for (float v : pos)
        if (!sigma_ok(v)) return fail(c, FOVPT_E_INVALID, "%s: key, exposure or white %g outside [%g, %g]", who, (double)v, (double)FOVPT_SIGMA_MIN, (double)FOVPT_SIGMA_MAX);
    const float rates[2] = {ec->adapt_brighter, ec->adapt_darker};
    for (float v : rates)
        if (!(v > 0.0f && v <= 1.0f)) return fail(c, FOVPT_E_INVALID, "%s: adapt rate %g outside (0, 1]", who, (double)v);
    CHK(check_reserved(c, &ec->_reserved0, 1, who));
    CHK(check_reserved(c, ec->_reserved, sizeof(ec->_reserved) / 4, who));
    CHK(check_rendered_frame(c, lp, who, "meter", nullptr, 1ull << 31));
    if (!in) return fail(c, FOVPT_E_INVALID, "%s: null accum_buffer", who);
    return FOVPT_OK;
}

ExposeArgs expose_args(const fovpt_expose_config* ec, const fovpt_ctx::Rendered& R)
{
    ExposeArgs a;
    memset(&a, 0, sizeof(a));
    a.weight[0] = ec->weight_fovea; a.weight[1] = ec->weight_middle; a.weight[2] = ec->weight_periphery; a.weight[3] = ec->weight_uniform;
    a.uniform = R.uniform != 0;
    a.low = ec->low_permille; a.high = ec->high_permille;
    a.ev_min = ec->ev_min; a.ev_max = ec->ev_max; a.key = ec->key;
    a.adapt_brighter = ec->adapt_brighter; a.adapt_darker = ec->adapt_darker;
    a.tone = ec->tone; a.white = ec->white; a.exposure = ec->exposure;
    return a;
}

// AUTO: the state (made on first use) and the meter's rows and histogram, k_expose_meter, k_expose_adapt; then k_expose_apply
int expose_enqueue(fovpt_ctx* c, const fovpt_expose_config* ec, const fovpt_float4* in, fovpt_float4* out_color, uint32_t* out_rgba)
{
    fovpt_ctx::Expose& E = c->expose;
    const size_t npix = c->rendered.pixels();
    const bool aut = ec->mode == FOVPT_EXPOSE_AUTO;
    const uint32_t nrows = fovpt_expose_rows(npix);
    const ExposeArgs a = expose_args(ec, c->rendered);
    const hipStream_t st = c->shadow_stream;
    if (aut) {
        CHK(record_make(c, E.state, sizeof(ExposeState)));
        HIPCHK(c, E.rows.reserve((size_t)nrows * FOVPT_EXPOSE_BINS * sizeof(uint32_t)));
        HIPCHK(c, E.hist.reserve(FOVPT_EXPOSE_BINS * sizeof(uint64_t)));
        fovpt_launch_expose_meter(st, c->rendered.frame, a, ec->metering == FOVPT_METER_GAZE, in, (uint32_t*)E.rows.p);
        fovpt_launch_expose_adapt(st, a, (const uint32_t*)E.rows.p, nrows, (uint64_t*)E.hist.p, (ExposeState*)E.state.p);
    }
    fovpt_launch_expose_apply(st, npix, a, aut ? (const ExposeState*)E.state.p : nullptr, in, out_color, out_rgba);
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

// ---- fovpt_warp and fovpt_warp_motion --------------------------------------------------------------------------------------------
// the validation both share, in fovpt_warp's order; makes the scatter's arguments (the camera's inverse and eye: all there is to
// them, and a singular camera has none).  reserved: the config's nres words; in, rin: the inputs of the enabled images (null: not enabled)
// the part of it that fovpt_warp_depth shares: the images, the fill radius and the reserved words of a config ...
int warp_config_check(fovpt_ctx* c, int32_t images, int32_t fill_radius, const int32_t* reserved, int nres, const char* who)
{
    if (images == 0 || (images & ~(FOVPT_WARP_COLOR | FOVPT_WARP_RGBA)))
        return fail(c, FOVPT_E_INVALID, "%s: images %d names no image or an unknown one", who, images);
    if (fill_radius < 0 || fill_radius > FOVPT_WARP_MAX_RADIUS)
        return fail(c, FOVPT_E_INVALID, "%s: fill_radius %d outside 0 .. %d", who, fill_radius, FOVPT_WARP_MAX_RADIUS);
    return check_reserved(c, reserved, nres, who);
}

// ... and a camera (`which`: "to warp to", "the depths were rendered with"): finite, with an inverse, which goes to inv
int warp_camera_check(fovpt_ctx* c, const fovpt_warp_camera* cam, const char* which, const char* who, float* inv)
{
    for (int k = 0; k < 12; k++)                                           // eye, U, V, W: 12 floats
        if (!std::isfinite((&cam->eye.x)[k])) return fail(c, FOVPT_E_INVALID, "%s: the camera %s has a non-finite entry", who, which);
    if (!camera_inverse(&cam->U.x, &cam->V.x, &cam->W.x, inv)) return fail(c, FOVPT_E_INVALID, "%s: the camera %s is singular", who, which);
    return FOVPT_OK;
}

int warp_check(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_warp_camera* to, int32_t images, int32_t fill_radius, const int32_t* reserved,
               int nres, const fovpt_gbuffer_ptrs* gbuffer, const fovpt_float4* in, const uint32_t* rin, const char* who, WarpArgs& a)
{
    CHK(warp_config_check(c, images, fill_radius, reserved, nres, who));
    memset(&a, 0, sizeof(a));
    CHK(warp_camera_check(c, to, "to warp to", who, a.inv));
    memcpy(a.eye, &to->eye.x, sizeof(a.eye));
    if (!gbuffer && (!c->has_scene || lp->traversable != c->scene_id)) return fail(c, FOVPT_E_NO_SCENE, "%s without a scene", who);
    CHK(check_rendered_frame(c, lp, who, "warp", nullptr, 1ull << 30));
    if (gbuffer && (gbuffer->width != c->rendered.w || gbuffer->height != c->rendered.h || !gbuffer->prim || !gbuffer->position))
        return fail(c, FOVPT_E_INVALID, "%s: the G-buffer is not of the frame's size %d x %d, or has a null prim or position", who, c->rendered.w, c->rendered.h);
    if (((images & FOVPT_WARP_COLOR) && !in) || ((images & FOVPT_WARP_RGBA) && !rin)) return fail(c, FOVPT_E_INVALID, "%s: an enabled image has a null input", who);
    return FOVPT_OK;
}

// Enqueued on fovpt_stream() like fovpt_denoise, and ordered like it.  Without a caller's G-buffer the rendered frame's first (the
// same stream, into fovpt_gbuffer's buffers); then the keys and counts are cleared, k_warp_scatter (motion null) or
// k_warp_scatter_motion (motion: its advance; the rest is filled in here, behind the trace), k_warp_resolve.
int warp_enqueue(fovpt_ctx* c, const fovpt_launch_params* lp, const WarpArgs& a, GBufferDev g, bool trace, int32_t fill_radius, const float* motion,
                 const fovpt_float4* in, const uint32_t* rin, fovpt_float4* out_color, uint32_t* out_rgba, uint32_t* out_map, const char* who)
{
    if (trace) CHK(enqueue_gbuffer(c, lp, c->rendered.frame, g, who));     // the rendered frame's camera
    const fovpt_ctx::Rendered& R = c->rendered;
    const hipStream_t st = c->shadow_stream;
    uint64_t *keys = (uint64_t*)c->warp.keys.p, *counts = (uint64_t*)c->warp.counts.p;
    HIPCHK(c, hipMemsetAsync(keys, 0xff, R.pixels() * 8, st));
    HIPCHK(c, hipMemsetAsync(counts, 0, FOVPT_WARP_COUNT_BYTES, st));
    if (!motion) fovpt_launch_warp_scatter(st, R.frame, a, g.prim, g.pos, keys, counts);
    else {
        WarpMotionArgs m;
        memset(&m, 0, sizeof(m));
        m.hit = (const float4*)c->gbuffer.hit.p; m.tris = c->tris;
        m.mark = (const uint64_t*)c->tm_mark.p; m.epoch = c->tm_epoch - 1;     // the step that ended the last interval
        m.tri_vidx = (const uint3*)c->up_vidx.p; m.vtx_prev = (const float*)c->vtx_prev.p;
        m.tri_bytes = (uint64_t)c->num_tris * sizeof(TriRec);
        m.num_prims = (uint32_t)(c->h_tri_vidx.size() / 3); m.num_meshes = (uint32_t)c->mesh_nv.size();
        m.advance = *motion;
        fovpt_launch_warp_scatter_motion(st, R.frame, a, m, g.prim, g.pos, keys, counts);
    }
    fovpt_launch_warp_resolve(st, R.w, R.h, fill_radius, keys, in, rin, out_color, out_rgba, out_map, counts);
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

// fovpt_warp (advance null) and fovpt_warp_motion, behind their null checks
int warp_call(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_warp_camera* to, int32_t images, int32_t fill_radius, const int32_t* reserved, int nres,
              const float* advance, const fovpt_gbuffer_ptrs* gbuffer, const fovpt_float4* in_color, const uint32_t* in_rgba, fovpt_float4* out_color,
              uint32_t* out_rgba, uint32_t* out_map, const char* who)
{
    if (advance && !(*advance >= 0.0f && *advance <= FOVPT_WARP_MAX_ADVANCE))   // (NaN fails)
        return fail(c, FOVPT_E_INVALID, "%s: advance %g outside 0 .. %g", who, (double)*advance, (double)FOVPT_WARP_MAX_ADVANCE);
    const bool C_ = images & FOVPT_WARP_COLOR, R_ = images & FOVPT_WARP_RGBA;
    const fovpt_float4* in = C_ ? (in_color ? in_color : lp->frame.accum_buffer) : nullptr;
    const uint32_t* rin = R_ ? (in_rgba ? in_rgba : lp->frame.frame_buffer) : nullptr;
    WarpArgs a;
    CHK(warp_check(c, lp, to, images, fill_radius, reserved, nres, gbuffer, in, rin, who, a));
    if (advance) {                                                         // fovpt_warp_motion: the last temporal step, the previous positions and the hit records describe the rendered frame
        if (!c->temporal.valid) return fail(c, FOVPT_E_NO_FRAME, "%s: no temporal step since create / reset / resize / set_scene", who);
        if (!c->tm_tracking)
            return fail(c, FOVPT_E_NO_FRAME, "%s: previous positions are not tracked yet (no fovpt_temporal_motion or fovpt_post with MOTION on this scene)", who);
        if (c->seq_update > c->seq_step)
            return fail(c, FOVPT_E_NO_FRAME, "%s: a geometry update has been issued since the last temporal step", who);
        if (gbuffer && !(c->gb_stamp > c->seq_frame && c->gb_stamp > c->seq_update && c->gb_stamp > c->seq_adopt))
            return fail(c, FOVPT_E_NO_FRAME, "%s: the context's last G-buffer trace is not of the rendered frame and the current geometry "
                                             "(its hit records go with the caller's G-buffer)", who);
    }
    // the buffers -- the context's own outputs where an enabled image has none, the keys, the counts -- and the last of the validation,
    // which needs them: no output is an input, the keys or another output (the resolve reads other pixels' inputs and keys while it writes)
    HIPCHK(c, hipSetDevice(c->device));
    fovpt_ctx::Warp& W = c->warp;
    const size_t npix = c->rendered.pixels();
    if (!C_) out_color = nullptr;
    else if (!out_color) { HIPCHK(c, W.out.color.reserve(npix * 16)); out_color = (fovpt_float4*)W.out.color.p; }
    if (!R_) out_rgba = nullptr;
    else if (!out_rgba) { HIPCHK(c, W.out.rgba.reserve(npix * 4)); out_rgba = (uint32_t*)W.out.rgba.p; }
    HIPCHK(c, W.keys.reserve(npix * 8));
    CHK(record_make(c, W.counts, FOVPT_WARP_COUNT_BYTES));
    const GBufferDev g = gbuffer_dev(c, gbuffer);                          // (the context's own: null until the first trace)
    CHK(check_aliases(c, {out_color, out_rgba, out_map}, {in, rin, g.prim, g.pos, W.keys.p}, who, "%s: an output is an input of the call (the resolve reads across pixels)"));
    // what the host knows: with no mesh moved in the interval, a step that did not see its updates, or no advance, fovpt_warp's scatter
    bool moved = false;
    if (advance && !c->tm_step_blind && *advance != 0.0f)
        for (const uint64_t e : c->tm_mesh_epoch) moved = moved || e == c->tm_epoch - 1;
    return warp_enqueue(c, lp, a, g, !gbuffer, fill_radius, moved ? advance : nullptr, in, rin, out_color, out_rgba, out_map, who);
}

// ---- fovpt_focus -----------------------------------------------------------------------------------------------------------------
// in: its colour input
int focus_check(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_focus_config* fc, const fovpt_gbuffer_ptrs* gbuffer, const fovpt_float4* in,
                const char* who)
{
    if (fc->mode != FOVPT_FOCUS_FIXED && fc->mode != FOVPT_FOCUS_AUTO) return fail(c, FOVPT_E_INVALID, "%s: unknown mode %d", who, fc->mode);
    if (fc->meter_radius < 0 || fc->meter_radius > FOVPT_FOCUS_MAX_METER_RADIUS)
        return fail(c, FOVPT_E_INVALID, "%s: meter_radius %d outside 0 .. %d", who, fc->meter_radius, FOVPT_FOCUS_MAX_METER_RADIUS);
    if (fc->rank_permille < 0 || fc->rank_permille > 1000) return fail(c, FOVPT_E_INVALID, "%s: rank_permille %d outside 0 .. 1000", who, fc->rank_permille);
    if (fc->max_radius < 0 || fc->max_radius > FOVPT_FOCUS_MAX_RADIUS)
        return fail(c, FOVPT_E_INVALID, "%s: max_radius %d outside 0 .. %d", who, fc->max_radius, FOVPT_FOCUS_MAX_RADIUS);
    if (!(fc->strength >= 0.0f && fc->strength <= FOVPT_SIGMA_MAX)) return fail(c, FOVPT_E_INVALID, "%s: strength %g outside [0, %g]", who, (double)fc->strength, (double)FOVPT_SIGMA_MAX);
    const float dist[2] = {fc->focus_distance, fc->focus_default};
    for (float v : dist)
        if (!sigma_ok(v)) return fail(c, FOVPT_E_INVALID, "%s: focus distance %g outside [%g, %g]", who, (double)v, (double)FOVPT_SIGMA_MIN, (double)FOVPT_SIGMA_MAX);
    const float rates[2] = {fc->adapt_nearer, fc->adapt_farther};
    for (float v : rates)
        if (!(v > 0.0f && v <= 1.0f)) return fail(c, FOVPT_E_INVALID, "%s: adapt rate %g outside (0, 1]", who, (double)v);
    CHK(check_reserved(c, fc->_reserved, sizeof(fc->_reserved) / 4, who));
    if (!gbuffer && (!c->has_scene || lp->traversable != c->scene_id)) return fail(c, FOVPT_E_NO_SCENE, "%s without a scene", who);
    CHK(check_rendered_frame(c, lp, who, "gather from", nullptr, 1ull << 31));
    if (gbuffer && (gbuffer->width != c->rendered.w || gbuffer->height != c->rendered.h || !gbuffer->prim || !gbuffer->position))
        return fail(c, FOVPT_E_INVALID, "%s: the G-buffer is not of the frame's size %d x %d, or has a null prim or position", who, c->rendered.w, c->rendered.h);
    if (!in) return fail(c, FOVPT_E_INVALID, "%s: null accum_buffer", who);
    return FOVPT_OK;
}

// the meter's square about the rendered gaze, clipped to the frame, and the config
FocusArgs focus_args(const fovpt_focus_config* fc, const fovpt_ctx::Rendered& Rd)
{
    FocusArgs a;
    memset(&a, 0, sizeof(a));
    a.cx = (int64_t)Rd.frame.cx; a.cy = (int64_t)Rd.frame.cy;             // (frame.c is unsigned: no difference below wraps)
    const int64_t R = fc->meter_radius;
    const int64_t x0 = a.cx - R > 0 ? a.cx - R : 0, x1 = a.cx + R < Rd.w - 1 ? a.cx + R : Rd.w - 1;
    const int64_t y0 = a.cy - R > 0 ? a.cy - R : 0, y1 = a.cy + R < Rd.h - 1 ? a.cy + R : Rd.h - 1;
    if (x0 <= x1 && y0 <= y1) { a.x0 = (int32_t)x0; a.x1 = (int32_t)x1; a.y0 = (int32_t)y0; a.y1 = (int32_t)y1; }
    else { a.x0 = a.y0 = 0; a.x1 = a.y1 = -1; }                            // the disc's square misses the frame
    a.meter_radius = fc->meter_radius; a.rank_permille = fc->rank_permille; a.max_radius = fc->max_radius;
    a.strength = fc->strength; a.focus_default = fc->focus_default;
    a.adapt_nearer = fc->adapt_nearer; a.adapt_farther = fc->adapt_farther;
    a.inv_focus = 1.0f / fc->focus_distance;
    return a;
}

// Without a caller's G-buffer (trace) the rendered frame's first (the same stream, into fovpt_gbuffer's buffers).  AUTO:
// k_focus_meter, k_focus_radius, k_focus_gather; the focus goes from the first to the second through the state record, never through
// the host.  FIXED: the last two.
int focus_enqueue(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_focus_config* fc, GBufferDev g, bool trace, const fovpt_float4* in,
                  fovpt_float4* out_color, uint32_t* out_rgba, float* out_coc, const char* who)
{
    if (trace) CHK(enqueue_gbuffer(c, lp, c->rendered.frame, g, who));     // the rendered frame's camera
    const fovpt_ctx::Rendered& R = c->rendered;
    const FocusArgs a = focus_args(fc, R);
    const hipStream_t st = c->shadow_stream;
    FocusState* state = fc->mode == FOVPT_FOCUS_AUTO ? (FocusState*)c->focus.state.p : nullptr;      // (AUTO: made by the entry point)
    float2* rt = (float2*)c->focus.rt.p;
    if (state) fovpt_launch_focus_meter(st, R.w, a, g.prim, g.pos, state);
    fovpt_launch_focus_radius(st, R.pixels(), a, state, g.prim, g.pos, rt, out_coc);
    fovpt_launch_focus_gather(st, R.w, R.h, fc->max_radius, in, rt, out_color, out_rgba);
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

// ---- fovpt_lens ------------------------------------------------------------------------------------------------------------------
// the config, and with `to` the re-aim H = M [U_to V_to W_to], M the inverse of the rendered camera.  false: that camera is singular
bool lens_args(const fovpt_lens_config* lc, const fovpt_warp_camera* to, const fovpt_ctx::Rendered& R, LensArgs& a)
{
    memset(&a, 0, sizeof(a));
    if (to) {
        float M[9];
        if (!camera_inverse(R.frame.U, R.frame.V, R.frame.W, M)) return false;
        const float* B[3] = {&to->U.x, &to->V.x, &to->W.x};               // the columns
        for (int k = 0; k < 3; k++)
            for (int j = 0; j < 3; j++)
                a.H[3 * k + j] = (float)(((double)M[3 * k] * (double)B[j][0] + (double)M[3 * k + 1] * (double)B[j][1]) + (double)M[3 * k + 2] * (double)B[j][2]);
        a.reaim = 1;
    }
    a.filter = lc->filter; a.encode = lc->encode;
    a.mono = memcmp(&lc->chroma[0], &lc->chroma[1], 4) == 0 && memcmp(&lc->chroma[0], &lc->chroma[2], 4) == 0;
    memcpy(a.center, lc->center, sizeof(a.center)); memcpy(a.scale, lc->scale, sizeof(a.scale));
    memcpy(a.k, lc->k, sizeof(a.k)); memcpy(a.chroma, lc->chroma, sizeof(a.chroma));
    a.clip_r2 = lc->clip_r2;
    memcpy(a.src_center, lc->src_center, sizeof(a.src_center)); memcpy(a.src_scale, lc->src_scale, sizeof(a.src_scale));
    memcpy(a.border, lc->border, sizeof(a.border));
    return true;
}

// makes the kernel's arguments.  in: its colour input
int lens_check(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_lens_config* lc, const fovpt_warp_camera* to, const fovpt_float4* in, const char* who,
               LensArgs& a)
{
    if (lc->filter != FOVPT_LENS_NEAREST && lc->filter != FOVPT_LENS_BILINEAR && lc->filter != FOVPT_LENS_BICUBIC)
        return fail(c, FOVPT_E_INVALID, "%s: unknown filter %d", who, lc->filter);
    if (lc->encode != FOVPT_LENS_ENCODE_DISPLAY && lc->encode != FOVPT_LENS_ENCODE_RESOLVE) return fail(c, FOVPT_E_INVALID, "%s: unknown encode %d", who, lc->encode);
    CHK(check_reserved(c, lc->_reserved0, sizeof(lc->_reserved0) / 4, who));
    CHK(check_reserved(c, lc->_reserved, sizeof(lc->_reserved) / 4, who));
    const float fields[19] = {lc->center[0], lc->center[1], lc->scale[0], lc->scale[1], lc->k[0], lc->k[1], lc->k[2], lc->k[3], lc->chroma[0], lc->chroma[1],
                              lc->chroma[2], lc->src_center[0], lc->src_center[1], lc->src_scale[0], lc->src_scale[1], lc->border[0], lc->border[1],
                              lc->border[2], lc->border[3]};
    for (float v : fields)
        if (!std::isfinite(v)) return fail(c, FOVPT_E_INVALID, "%s: a non-finite center, scale, k, chroma, src_* or border entry", who);
    if (!(lc->clip_r2 > 0.0f)) return fail(c, FOVPT_E_INVALID, "%s: clip_r2 %g is not above 0", who, (double)lc->clip_r2);
    for (int k = 0; to && k < 12; k++)                                     // eye, U, V, W: 12 floats
        if (!std::isfinite((&to->eye.x)[k])) return fail(c, FOVPT_E_INVALID, "%s: the camera to re-aim at has a non-finite entry", who);
    CHK(check_rendered_frame(c, lp, who, "resample", nullptr, 1ull << 31));
    if (!lens_args(lc, to, c->rendered, a)) return fail(c, FOVPT_E_INVALID, "%s: the rendered camera is singular", who);
    if (!in) return fail(c, FOVPT_E_INVALID, "%s: null accum_buffer", who);
    return FOVPT_OK;
}

// ---- fovpt_quality ---------------------------------------------------------------------------------------------------------------
// test: its test image
int quality_check(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_quality_config* qc, const uint32_t* test, const uint32_t* ref, const char* who)
{
    if (qc->flags & ~(FOVPT_QUALITY_SSIM | FOVPT_QUALITY_PROFILE)) return fail(c, FOVPT_E_INVALID, "%s: unknown flag bits 0x%x", who, (unsigned)qc->flags);
    if (qc->ring_width < 1 || qc->ring_width > FOVPT_QUALITY_MAX_RING_WIDTH)
        return fail(c, FOVPT_E_INVALID, "%s: ring_width %d outside 1 .. %d", who, qc->ring_width, FOVPT_QUALITY_MAX_RING_WIDTH);
    CHK(check_reserved(c, qc->_reserved, sizeof(qc->_reserved) / 4, who));
    CHK(check_rendered_frame(c, lp, who, "measure", nullptr, 1ull << 31));
    if (!ref) return fail(c, FOVPT_E_INVALID, "%s: null reference image", who);
    if (!test) return fail(c, FOVPT_E_INVALID, "%s: null frame_buffer", who);
    return FOVPT_OK;
}

// the measurement's buffers and launches for a checked call (out_sums null: the context's own record)
int quality_enqueue(fovpt_ctx* c, const fovpt_quality_config* qc, const uint32_t* test, const uint32_t* ref, fovpt_quality_sums* out_sums, uint8_t* out_class)
{
    const fovpt_ctx::Rendered& R = c->rendered;
    if (!out_sums) {
        HIPCHK(c, c->quality.sums.reserve(sizeof(fovpt_quality_sums)));     // (made here, and the launch below writes every byte of it)
        out_sums = (fovpt_quality_sums*)c->quality.sums.p;
    }
    HIPCHK(c, c->quality.rows.reserve((size_t)fovpt_quality_rows(R.w, R.h) * FOVPT_QUALITY_COLUMNS * sizeof(uint64_t)));
    QualityArgs a;
    memset(&a, 0, sizeof(a));
    a.cx = (int64_t)(int32_t)R.frame.cx; a.cy = (int64_t)(int32_t)R.frame.cy;      // the rendered gaze
    a.flags = qc->flags; a.ring_width = qc->ring_width;
    a.uniform = R.uniform != 0;
    fovpt_launch_quality(c->shadow_stream, R.frame, a, test, ref, (uint64_t*)c->quality.rows.p, out_sums, out_class);
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

}  // namespace

extern "C" {

// ---- gaze-metered auto-exposure and tone map (expose.hip; its definition: tests/expose_ref.py) ---------------------------
// (conventions, not measurements: include/fovpt.h)
int fovpt_expose_defaults(fovpt_expose_config* out)
{
    if (!zeroed(out)) return FOVPT_E_INVALID;
    out->mode = FOVPT_EXPOSE_AUTO;
    out->metering = FOVPT_METER_GAZE;
    out->tone = FOVPT_TONE_REINHARD;
    out->weight_fovea = 64; out->weight_middle = 8; out->weight_periphery = 1; out->weight_uniform = 1;
    out->low_permille = 100; out->high_permille = 950;
    out->ev_min = -12.0f; out->ev_max = 12.0f;
    out->key = 0.18f;
    out->exposure = 16.0f;
    out->white = FOVPT_SIGMA_MAX;
    out->adapt_brighter = 1.0f; out->adapt_darker = 1.0f;
    return FOVPT_OK;
}

int fovpt_expose_buffers(fovpt_ctx* c, fovpt_float4** color, uint32_t** rgba)
{
    return c ? own_buffers(c, "fovpt_expose_buffers", c->expose.out, color, rgba) : FOVPT_E_INVALID;
}

int fovpt_expose_state(fovpt_ctx* c, struct fovpt_expose_state* out)
{
    return c ? record_read(c, c->expose.state, out, sizeof(*out), "fovpt_expose_state: null argument") : FOVPT_E_INVALID;   // (zeros: no step yet)
}

int fovpt_expose_reset(fovpt_ctx* c)
{
    if (!c) return FOVPT_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    return record_reset(c, c->expose.state, sizeof(ExposeState), c->shadow_stream);     // steps = 0: the next AUTO step is a first step
}

// Enqueued on fovpt_stream() like fovpt_denoise, and ordered like it.  AUTO: k_expose_meter, k_expose_adapt, k_expose_apply; the
// exposure goes from the second to the third through the state record, never through the host.  FIXED: k_expose_apply alone.
int fovpt_expose(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_expose_config* ec, const fovpt_float4* in_color, fovpt_float4* out_color,
                 uint32_t* out_rgba)
{
    const char* who = "fovpt_expose";
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !ec) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    const fovpt_float4* in = in_color ? in_color : lp->frame.accum_buffer;
    CHK(expose_check(c, lp, ec, in, who));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(own_outputs(c, who, c->expose.out, out_color, out_rgba));
    return expose_enqueue(c, ec, in, out_color, out_rgba);
}

// ---- late reprojection of the finished frame to a newer camera (warp.hip; its definition: tests/warp_ref.py) ------------------
// (fill_radius: a convention, not a measurement: include/fovpt.h)
int fovpt_warp_defaults(fovpt_warp_config* out)
{
    if (!zeroed(out)) return FOVPT_E_INVALID;
    out->images = FOVPT_WARP_COLOR | FOVPT_WARP_RGBA;
    out->fill_radius = 2;
    return FOVPT_OK;
}

int fovpt_warp_buffers(fovpt_ctx* c, fovpt_float4** color, uint32_t** rgba)
{
    return c ? own_buffers(c, "fovpt_warp_buffers", c->warp.out, color, rgba) : FOVPT_E_INVALID;
}

int fovpt_warp_counts(fovpt_ctx* c, struct fovpt_warp_counts* out)
{
    if (!c) return FOVPT_E_INVALID;
    if (!out) return fail(c, FOVPT_E_INVALID, "fovpt_warp_counts: null argument");
    memset(out, 0, sizeof(*out));
    std::vector<uint64_t> part(FOVPT_WARP_COUNT_BYTES / sizeof(uint64_t));
    CHK(record_read(c, c->warp.counts, part.data(), FOVPT_WARP_COUNT_BYTES, nullptr));   // (zeros: no warp yet)
    for (size_t s = 0; s < FOVPT_WARP_COUNT_SLOTS; s++) {                  // the waves' partial records
        const uint64_t* p = &part[s * FOVPT_WARP_COUNT_STRIDE];
        out->splatted += p[0]; out->direct += p[1]; out->filled += p[2]; out->empty += p[3];
    }
    return FOVPT_OK;
}

int fovpt_warp(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_warp_camera* to, const fovpt_warp_config* wc, const fovpt_gbuffer_ptrs* gbuffer,
               const fovpt_float4* in_color, const uint32_t* in_rgba, fovpt_float4* out_color, uint32_t* out_rgba, uint32_t* out_map)
{
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !to || !wc) return fail(c, FOVPT_E_INVALID, "%s: null argument", "fovpt_warp");
    return warp_call(c, lp, to, wc->images, wc->fill_radius, wc->_reserved, 6, nullptr, gbuffer, in_color, in_rgba, out_color, out_rgba, out_map, "fovpt_warp");
}

// ---- fovpt_warp in which the meshes that moved in the last interval go on moving (warp.hip, k_warp_scatter_motion; its definition:
// tests/warp_motion_ref.py) ----------------------------------------------------------------------------
// (advance: a convention, not a measurement: include/fovpt.h)
int fovpt_warp_motion_defaults(fovpt_warp_motion_config* out)
{
    if (!zeroed(out)) return FOVPT_E_INVALID;
    out->images = FOVPT_WARP_COLOR | FOVPT_WARP_RGBA;
    out->fill_radius = 2;
    out->advance = 1.0f;
    return FOVPT_OK;
}

int fovpt_warp_motion(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_warp_camera* to, const fovpt_warp_motion_config* mc,
                      const fovpt_gbuffer_ptrs* gbuffer, const fovpt_float4* in_color, const uint32_t* in_rgba, fovpt_float4* out_color,
                      uint32_t* out_rgba, uint32_t* out_map)
{
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !to || !mc) return fail(c, FOVPT_E_INVALID, "%s: null argument", "fovpt_warp_motion");
    return warp_call(c, lp, to, mc->images, mc->fill_radius, mc->_reserved, 5, &mc->advance, gbuffer, in_color, in_rgba, out_color, out_rgba, out_map, "fovpt_warp_motion");
}

// ---- fovpt_warp from a depth image and two cameras, for a client that holds no scene and no rendered frame (warp.hip,
// k_warp_scatter_depth; its definition: tests/warp_depth_ref.py) -------------------------------------------
// Enqueued on fovpt_stream(): the keys (the context's own for this call) and the counts are cleared, k_warp_scatter_depth, k_warp_resolve.
int fovpt_warp_depth(fovpt_ctx* c, int width, int height, const fovpt_warp_camera* from, const fovpt_warp_camera* to, const fovpt_warp_config* wc,
                     const float* depth, const fovpt_float4* in_color, const uint32_t* in_rgba, fovpt_float4* out_color, uint32_t* out_rgba,
                     uint32_t* out_map)
{
    const char* who = "fovpt_warp_depth";
    if (!c) return FOVPT_E_INVALID;
    if (!from || !to || !wc || !depth) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    if (width < 1 || height < 1 || (uint64_t)width * (uint64_t)height >= (1ull << 30))
        return fail(c, FOVPT_E_INVALID, "%s: size %d x %d is empty or has 2^30 pixels or more", who, width, height);
    CHK(warp_config_check(c, wc->images, wc->fill_radius, wc->_reserved, 6, who));
    WarpArgs a;
    memset(&a, 0, sizeof(a));
    float from_inv[9];
    CHK(warp_camera_check(c, to, "to warp to", who, a.inv));
    CHK(warp_camera_check(c, from, "the depths were rendered with", who, from_inv));
    memcpy(a.eye, &to->eye.x, sizeof(a.eye));
    const bool C_ = wc->images & FOVPT_WARP_COLOR, R_ = wc->images & FOVPT_WARP_RGBA;
    if ((C_ && (!in_color || !out_color)) || (R_ && (!in_rgba || !out_rgba)))
        return fail(c, FOVPT_E_INVALID, "%s: an enabled image has a null input or a null output", who);
    if (!C_) { in_color = nullptr; out_color = nullptr; }
    if (!R_) { in_rgba = nullptr; out_rgba = nullptr; }
    HIPCHK(c, hipSetDevice(c->device));
    fovpt_ctx::Warp& W = c->warp;
    const size_t npix = (size_t)width * (size_t)height;
    HIPCHK(c, W.depth_keys.reserve(npix * 8));
    CHK(record_make(c, W.counts, FOVPT_WARP_COUNT_BYTES));
    CHK(check_aliases(c, {out_color, out_rgba, out_map}, {in_color, in_rgba, depth, W.depth_keys.p}, who,
                      "%s: an output is an input of the call (the resolve reads across pixels)"));
    FrameDev fd;                                                           // the size and the camera: all the scatter reads of it
    memset(&fd, 0, sizeof(fd));
    fd.w = width; fd.h = height;
    memcpy(fd.eye, &from->eye.x, sizeof(fd.eye)); memcpy(fd.U, &from->U.x, sizeof(fd.U));
    memcpy(fd.V, &from->V.x, sizeof(fd.V)); memcpy(fd.W, &from->W.x, sizeof(fd.W));
    const hipStream_t st = c->shadow_stream;
    uint64_t *keys = (uint64_t*)W.depth_keys.p, *counts = (uint64_t*)W.counts.p;
    HIPCHK(c, hipMemsetAsync(keys, 0xff, npix * 8, st));
    HIPCHK(c, hipMemsetAsync(counts, 0, FOVPT_WARP_COUNT_BYTES, st));
    fovpt_launch_warp_scatter_depth(st, fd, a, depth, keys, counts);
    fovpt_launch_warp_resolve(st, width, height, wc->fill_radius, keys, in_color, in_rgba, out_color, out_rgba, out_map, counts);
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

// ---- gaze-metered focus distance and depth of field (focus.hip; its definition: tests/focus_ref.py) ---------------------------
// (conventions, not measurements: include/fovpt.h)
int fovpt_focus_defaults(fovpt_focus_config* out)
{
    if (!zeroed(out)) return FOVPT_E_INVALID;
    out->mode = FOVPT_FOCUS_AUTO;
    out->meter_radius = 12;
    out->rank_permille = 250;
    out->max_radius = 6;
    out->strength = 8.0f;
    out->focus_distance = 1.0f;
    out->focus_default = 1.0f;
    out->adapt_nearer = 1.0f; out->adapt_farther = 1.0f;
    return FOVPT_OK;
}

int fovpt_focus_buffers(fovpt_ctx* c, fovpt_float4** color, uint32_t** rgba)
{
    return c ? own_buffers(c, "fovpt_focus_buffers", c->focus.out, color, rgba) : FOVPT_E_INVALID;
}

int fovpt_focus_state(fovpt_ctx* c, struct fovpt_focus_state* out)
{
    return c ? record_read(c, c->focus.state, out, sizeof(*out), "fovpt_focus_state: null argument") : FOVPT_E_INVALID;   // (zeros: no AUTO step yet)
}

int fovpt_focus_reset(fovpt_ctx* c)
{
    if (!c) return FOVPT_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    return record_reset(c, c->focus.state, sizeof(FocusState), c->shadow_stream);       // steps = 0: the next AUTO step is a first step
}

// Enqueued on fovpt_stream() like fovpt_denoise, and ordered like it (focus_enqueue).
int fovpt_focus(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_focus_config* fc, const fovpt_gbuffer_ptrs* gbuffer,
                const fovpt_float4* in_color, fovpt_float4* out_color, uint32_t* out_rgba, float* out_coc)
{
    const char* who = "fovpt_focus";
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !fc) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    const fovpt_float4* in = in_color ? in_color : lp->frame.accum_buffer;
    CHK(focus_check(c, lp, fc, gbuffer, in, who));
    // buffers: the context's own outputs where the caller gave none, the (r, tp) pairs, the state
    HIPCHK(c, hipSetDevice(c->device));
    CHK(own_outputs(c, who, c->focus.out, out_color, out_rgba));
    HIPCHK(c, c->focus.rt.reserve(c->rendered.pixels() * 8));
    if (fc->mode == FOVPT_FOCUS_AUTO) CHK(record_make(c, c->focus.state, sizeof(FocusState)));
    // the gather reads other pixels' colours and pairs while it writes, the radius pass the G-buffer: no output is one of them
    const GBufferDev g = gbuffer_dev(c, gbuffer);                          // (the context's own: null until the first trace)
    CHK(check_aliases(c, {out_color, out_rgba, out_coc}, {in, g.prim, g.pos, c->focus.rt.p}, who, "%s: an output is an input of the call (the gather reads across pixels)"));
    return focus_enqueue(c, lp, fc, g, !gbuffer, in, out_color, out_rgba, out_coc, who);
}

// ---- head-mounted display lens pre-distortion (lens.hip; its definition: tests/lens_ref.py) ---------------------------------------
// (conventions, not measurements: include/fovpt.h)
int fovpt_lens_defaults(fovpt_lens_config* out)
{
    if (!zeroed(out)) return FOVPT_E_INVALID;
    out->filter = FOVPT_LENS_BILINEAR;
    out->encode = FOVPT_LENS_ENCODE_DISPLAY;
    out->scale[0] = out->scale[1] = 1.0f;
    out->k[0] = 1.0f; out->k[1] = 0.22f; out->k[2] = 0.24f; out->k[3] = 0.0f;
    out->chroma[0] = 0.996f; out->chroma[1] = 1.0f; out->chroma[2] = 1.014f;
    out->clip_r2 = INFINITY;
    out->src_scale[0] = out->src_scale[1] = 1.0f;
    out->border[3] = 1.0f;
    return FOVPT_OK;
}

int fovpt_lens_buffers(fovpt_ctx* c, fovpt_float4** color, uint32_t** rgba)
{
    return c ? own_buffers(c, "fovpt_lens_buffers", c->lens.out, color, rgba) : FOVPT_E_INVALID;
}

// Enqueued on fovpt_stream() like fovpt_denoise, and ordered like it: one launch of k_lens.
int fovpt_lens(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_lens_config* lc, const fovpt_warp_camera* to, const fovpt_float4* in_color,
               fovpt_float4* out_color, uint32_t* out_rgba)
{
    const char* who = "fovpt_lens";
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !lc) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    const fovpt_float4* in = in_color ? in_color : lp->frame.accum_buffer;
    LensArgs a;
    CHK(lens_check(c, lp, lc, to, in, who, a));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(own_outputs(c, who, c->lens.out, out_color, out_rgba));
    CHK(check_aliases(c, {out_color, out_rgba}, {in}, who, "%s: an output is the input of the call (the gather reads across pixels)"));
    fovpt_launch_lens(c->shadow_stream, c->rendered.w, c->rendered.h, a, in, out_color, out_rgba);      // (all there is to enqueue)
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

// ---- image quality of the rendered frame (quality.hip; its definition: tests/quality_ref.py) -----------------------------------
// (ring_width: a convention, not a measurement: include/fovpt.h)
int fovpt_quality_defaults(fovpt_quality_config* out)
{
    if (!zeroed(out)) return FOVPT_E_INVALID;
    out->flags = FOVPT_QUALITY_SSIM | FOVPT_QUALITY_PROFILE;
    out->ring_width = 16;
    return FOVPT_OK;
}

// Enqueued on fovpt_stream() like fovpt_denoise, and ordered like it: k_quality_tile, k_quality_sum.  The rows between them are
// the context's; calls in flight use them one after the other, in stream order.
int fovpt_quality(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_quality_config* qc, const uint32_t* test_rgba, const uint32_t* ref_rgba,
                  fovpt_quality_sums* out_sums, uint8_t* out_class)
{
    const char* who = "fovpt_quality";
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !qc) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    const uint32_t* test = test_rgba ? test_rgba : lp->frame.frame_buffer;
    CHK(quality_check(c, lp, qc, test, ref_rgba, who));
    HIPCHK(c, hipSetDevice(c->device));
    return quality_enqueue(c, qc, test, ref_rgba, out_sums, out_class);
}

int fovpt_quality_read(fovpt_ctx* c, fovpt_quality_sums* out)
{
    // (zeros: no measurement into the context's record yet)
    return c ? record_read(c, c->quality.sums, out, sizeof(*out), "fovpt_quality_read: null argument") : FOVPT_E_INVALID;
}

}  // extern "C"
