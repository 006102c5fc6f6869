// api_post.hip -- post-processing of the rendered frame over the C ABI: fovpt_denoise (denoise.hip), fovpt_gbuffer /
// fovpt_reconstruct (reconstruct.hip), fovpt_temporal / fovpt_temporal_motion (temporal.hip), fovpt_expose (expose.hip), fovpt_warp /
// fovpt_warp_motion (warp.hip), fovpt_focus (focus.hip), fovpt_lens (lens.hip), fovpt_quality (quality.hip), and their defaults.
#include <cmath>
#include <cstring>

#include "fovpt_ctx.h"

namespace {

// an edge-stopping scale of fovpt_denoise / fovpt_reconstruct: inside [FOVPT_SIGMA_MIN, FOVPT_SIGMA_MAX], so that 1 / sigma^2
// is a normal float and the denoiser's colour scale (1 / sigma^2) * 4^(FOVPT_DENOISE_MAX_ITERATIONS - 1) / 1e-4 stays finite
// (an infinite scale makes the centre tap 0 * inf: every weight 0, the output 0 / 0)
bool sigma_ok(float v) { return v >= FOVPT_SIGMA_MIN && v <= FOVPT_SIGMA_MAX; }
float inv_sq(float s) { const float s2 = s * s; return 1.0f / s2; }

// What fovpt_denoise, fovpt_reconstruct and fovpt_temporal (`who`) ask of the frame last rendered: there is one, it has the guides
// where the call needs them (need_guides: the error text, or null), it is not a tile shard (a shard has no neighbours
// `to_what`), and lp's frame has its size.
int check_rendered_frame(fovpt_ctx* c, const fovpt_launch_params* lp, const char* who, const char* to_what, const char* need_guides)
{
    if (c->dn_w <= 0 || c->dn_h <= 0) return fail(c, FOVPT_E_NO_FRAME, "%s: no frame rendered yet", who);
    if (need_guides && (!c->dn_guides || c->any_catcher)) return fail(c, FOVPT_E_INVALID, "%s", need_guides);
    if (c->dn_world > 1) return fail(c, FOVPT_E_INVALID, "%s: a tile shard (world = %d) has no neighbours to %s", who, c->dn_world, to_what);
    if (lp->frame.size.x != c->dn_w || lp->frame.size.y != c->dn_h)
        return fail(c, FOVPT_E_NO_FRAME, "%s: frame size %d x %d differs from the last frame's %d x %d", who, lp->frame.size.x, lp->frame.size.y, c->dn_w, c->dn_h);
    return FOVPT_OK;
}

// The caller gave no output, or asks for the context's own (the *_buffers calls): the colour / rgba pair of the last frame's
// size, made on first use, for whichever of the two is null.
int own_outputs(fovpt_ctx* c, const char* who, DevBuf& color, DevBuf& rgba, fovpt_float4*& out_color, uint32_t*& out_rgba)
{
    if (out_color && out_rgba) return FOVPT_OK;
    if (!color.p) {
        if (c->dn_w <= 0 || c->dn_h <= 0) return fail(c, FOVPT_E_NO_FRAME, "%s: no frame rendered yet", who);
        HIPCHK(c, hipSetDevice(c->device));
    }
    const size_t n = (size_t)c->dn_w * (size_t)c->dn_h;
    HIPCHK(c, color.reserve(n * 16)); HIPCHK(c, rgba.reserve(n * 4));
    if (!out_color) out_color = (fovpt_float4*)color.p;
    if (!out_rgba) out_rgba = (uint32_t*)rgba.p;
    return FOVPT_OK;
}

GBufferDev temporal_set(fovpt_ctx* c, int k)
{
    GBufferDev g;
    g.prim = (uint32_t*)c->tp_prim[k].p; g.pos = (float4*)c->tp_pos[k].p; g.nrm = (float4*)c->tp_nrm[k].p; g.alb = (float4*)c->tp_alb[k].p;
    return g;
}

// The rows of [U V W]^-1 (U, V, W the columns), in binary64: det = U . (V x W), rows (V x W) / det, (W x U) / det,
// (U x V) / det, each entry rounded to binary32.  false: det is 0 or not finite.
bool camera_inverse(const float* U, const float* V, const float* W, float* inv)
{
    auto cross = [](const double* a, const double* b, double* r) {
        r[0] = a[1] * b[2] - a[2] * b[1]; r[1] = a[2] * b[0] - a[0] * b[2]; r[2] = a[0] * b[1] - a[1] * b[0];
    };
    const double u[3] = {U[0], U[1], U[2]}, v[3] = {V[0], V[1], V[2]}, w[3] = {W[0], W[1], W[2]};
    double r[3][3];
    cross(v, w, r[0]); cross(w, u, r[1]); cross(u, v, r[2]);
    const double det = (u[0] * r[0][0] + u[1] * r[0][1]) + u[2] * r[0][2];
    if (det == 0.0 || !std::isfinite(det)) return false;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) inv[3 * i + j] = (float)(r[i][j] / det);
    return true;
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
    { const int rc_ = check_rendered_frame(c, lp, who, "filter with", "fovpt_denoise needs the denoiser guides: the frame was rendered without fovpt_config.write_guides = 1 (not available with shadow-catcher materials)"); if (rc_) return rc_; }
    if (!lp->frame.color_buffer || !lp->frame.normal_buffer || !lp->frame.albedo_buffer) return fail(c, FOVPT_E_INVALID, "%s: null guide buffers", who);
    return FOVPT_OK;
}

// the denoiser's buffers and launches for a checked call; out_color / out_rgba are set
int denoise_enqueue(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_denoise_config* dc, fovpt_float4* out_color, uint32_t* out_rgba)
{
    const size_t npix = (size_t)c->dn_w * (size_t)c->dn_h;
    HIPCHK(c, c->dn_level.reserve(npix));
    HIPCHK(c, c->dn_i0.reserve(npix * 16));
    HIPCHK(c, c->dn_i1.reserve(npix * 16));

    // the level map: the passes fovpt_render ran for this frame
    const FrameDev& fd = c->dn_frame;
    DenoiseArgs a;
    memset(&a, 0, sizeof(a));
    if (c->dn_uniform) a.n_pass[0] = dc->iterations_uniform;
    else { a.n_pass[0] = dc->iterations_periphery; a.n_pass[1] = dc->iterations_middle; a.n_pass[2] = dc->iterations_fovea; }
    for (int p = 0; p < fd.npass; p++) a.iterations = a.n_pass[p] > a.iterations ? a.n_pass[p] : a.iterations;
    a.inv_c = inv_sq(dc->color_sigma); a.inv_n = inv_sq(dc->normal_sigma); a.inv_a = inv_sq(dc->albedo_sigma);
    fovpt_launch_denoise(c->shadow_stream, fd, a, lp->frame.color_buffer, lp->frame.normal_buffer, lp->frame.albedo_buffer,
                         (float4*)c->dn_i0.p, (float4*)c->dn_i1.p, (uint8_t*)c->dn_level.p, out_color, out_rgba);
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
    for (int32_t r : rc->_reserved)
        if (r != 0) return fail(c, FOVPT_E_INVALID, "%s: reserved fields must be 0", who);
    if (!c->has_scene || lp->traversable != c->scene_id) return fail(c, FOVPT_E_NO_SCENE, "%s without a scene", who);
    const char* need_guides = "fovpt_reconstruct with remodulate = 1 needs the albedo guide: the frame was rendered without fovpt_config.write_guides = 1 (not available with shadow-catcher materials)";
    { const int rc_ = check_rendered_frame(c, lp, who, "reconstruct from", rc->remodulate ? need_guides : nullptr); if (rc_) return rc_; }
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
    { const int rc_ = enqueue_gbuffer(c, lp, c->dn_frame, g, who); if (rc_) return rc_; }   // the rendered frame's camera
    fovpt_launch_reconstruct(c->shadow_stream, c->dn_frame, reconstruct_args(rc), in, lp->frame.albedo_buffer, g, out_color, out_rgba);
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
    for (int32_t r : tc->_reserved)
        if (r != 0) return fail(c, FOVPT_E_INVALID, "%s: reserved fields must be 0", who);
    if (!c->has_scene || lp->traversable != c->scene_id) return fail(c, FOVPT_E_NO_SCENE, "%s without a scene", who);
    { const int rc_ = check_rendered_frame(c, lp, who, "reproject from", nullptr); if (rc_) return rc_; }
    if (!in) return fail(c, FOVPT_E_INVALID, "%s: null accum_buffer", who);
    return FOVPT_OK;
}

// what a temporal step's outputs must not be (the histories exist: reserve_temporal)
int temporal_alias_check(fovpt_ctx* c, const fovpt_float4* in, const fovpt_float4* out_color, const uint32_t* out_rgba, const fovpt_float4* out_motion,
                         const char* who)
{
    if ((void*)out_color == c->tp_hist[0].p || (void*)out_color == c->tp_hist[1].p)
        return fail(c, FOVPT_E_INVALID, "%s: the output colour buffer is the context's history", who);
    if (out_motion && (out_motion == out_color || (void*)out_motion == (void*)out_rgba || out_motion == in || (void*)out_motion == c->tp_hist[0].p ||
                       (void*)out_motion == c->tp_hist[1].p))
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
    if (motion && !c->tm_tracking) {                                       // the marks: no mesh has moved yet (0 is no step's number)
        const size_t nmesh = c->mesh_nv.size();
        HIPCHK(c, c->tm_mark.reserve(nmesh * sizeof(uint64_t)));
        HIPCHK(c, hipMemsetAsync(c->tm_mark.p, 0, nmesh * sizeof(uint64_t), st));
        c->tm_mesh_epoch.assign(nmesh, 0ull);
        c->tm_tracking = true;
    }
    const int cur = c->tp_last ^ 1, prev = c->tp_last;
    const GBufferDev g = temporal_set(c, cur), gp = temporal_set(c, prev);
    GBufferDev gt;
    { const int rc_ = enqueue_gbuffer(c, lp, c->dn_frame, gt, who, &g); if (rc_) return rc_; }   // the rendered frame's camera
    const FrameDev& fd = c->dn_frame;
    TemporalArgs a;
    memset(&a, 0, sizeof(a));
    a.cap[0] = tc->history_fovea; a.cap[1] = tc->history_middle; a.cap[2] = tc->history_periphery; a.cap[3] = tc->history_uniform;
    a.normal_tol = tc->normal_tolerance; a.depth_tol = tc->depth_tolerance;
    a.uniform = c->dn_uniform != 0;
    a.reproject = c->tp_valid && c->tp_w == c->dn_w && c->tp_h == c->dn_h && camera_inverse(c->tp_U, c->tp_V, c->tp_W, a.inv);
    memcpy(a.eye_prev, c->tp_eye, sizeof(a.eye_prev));
    const float4* hist_prev = (const float4*)c->tp_hist[prev].p;
    float4* hist_out = (float4*)c->tp_hist[cur].p;
    TemporalMotionArgs m;
    memset(&m, 0, sizeof(m));
    if (motion) {
        if (c->tm_untracked) a.reproject = 0;                              // meshes moved unrecorded: where they were is not known
        m.hit = (const float4*)c->gb_hit.p; m.tris = c->tris;
        m.mark = (const uint64_t*)c->tm_mark.p; m.epoch = c->tm_epoch;
        m.tri_vidx = (const uint3*)c->up_vidx.p; m.vtx_prev = (const float*)c->vtx_prev.p;
        m.out_motion = out_motion;
    }
    if (fuse) fovpt_launch_reconstruct_temporal(st, fd, *fuse, a, motion ? &m : nullptr, in, lp->frame.albedo_buffer, g, gp, hist_prev, hist_out, out_color, out_rgba);
    else if (!motion) fovpt_launch_temporal(st, fd, a, in, g, gp, hist_prev, hist_out, out_color, out_rgba);
    else fovpt_launch_temporal_motion(st, fd, a, m, in, g, gp, hist_prev, hist_out, out_color, out_rgba);
    HIPCHK(c, hipGetLastError());
    c->tp_last = cur;                                                      // this step is the next one's previous step
    c->tp_valid = true;
    c->tp_w = c->dn_w; c->tp_h = c->dn_h;
    memcpy(c->tp_eye, fd.eye, sizeof(c->tp_eye)); memcpy(c->tp_U, fd.U, sizeof(c->tp_U));
    memcpy(c->tp_V, fd.V, sizeof(c->tp_V)); memcpy(c->tp_W, fd.W, sizeof(c->tp_W));
    c->tm_epoch++;                                                         // the marks of this interval no longer hold
    c->tm_step_blind = c->tm_untracked;                                    // fovpt_warp_motion: what this step knew of the interval it ended
    c->seq_step = ++c->seq;
    c->tm_untracked = false;
    return FOVPT_OK;
}

// fovpt_expose's validation (nothing allocated, enqueued or changed).  in: its colour input
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
    if (ec->_reserved0 != 0) return fail(c, FOVPT_E_INVALID, "%s: reserved fields must be 0", who);
    for (int32_t r : ec->_reserved)
        if (r != 0) return fail(c, FOVPT_E_INVALID, "%s: reserved fields must be 0", who);
    { const int rc_ = check_rendered_frame(c, lp, who, "meter", nullptr); if (rc_) return rc_; }
    if ((size_t)c->dn_w * (size_t)c->dn_h >= (1ull << 31)) return fail(c, FOVPT_E_INVALID, "%s: frame too large (%d x %d)", who, c->dn_w, c->dn_h);
    if (!in) return fail(c, FOVPT_E_INVALID, "%s: null accum_buffer", who);
    return FOVPT_OK;
}

// fovpt_quality's validation (nothing allocated, enqueued or changed).  test: its test image
int quality_check(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_quality_config* qc, const uint32_t* test, const uint32_t* ref, const char* who)
{
    if (qc->flags & ~(FOVPT_QUALITY_SSIM | FOVPT_QUALITY_PROFILE)) return fail(c, FOVPT_E_INVALID, "%s: unknown flag bits 0x%x", who, (unsigned)qc->flags);
    if (qc->ring_width < 1 || qc->ring_width > FOVPT_QUALITY_MAX_RING_WIDTH)
        return fail(c, FOVPT_E_INVALID, "%s: ring_width %d outside 1 .. %d", who, qc->ring_width, FOVPT_QUALITY_MAX_RING_WIDTH);
    for (int32_t r : qc->_reserved)
        if (r != 0) return fail(c, FOVPT_E_INVALID, "%s: reserved fields must be 0", who);
    { const int rc_ = check_rendered_frame(c, lp, who, "measure", nullptr); if (rc_) return rc_; }
    if ((size_t)c->dn_w * (size_t)c->dn_h >= (1ull << 31)) return fail(c, FOVPT_E_INVALID, "%s: frame too large (%d x %d)", who, c->dn_w, c->dn_h);
    if (!ref) return fail(c, FOVPT_E_INVALID, "%s: null reference image", who);
    if (!test) return fail(c, FOVPT_E_INVALID, "%s: null frame_buffer", who);
    return FOVPT_OK;
}

// the measurement's buffers and launches for a checked call (out_sums null: the context's own record)
int quality_enqueue(fovpt_ctx* c, const fovpt_quality_config* qc, const uint32_t* test, const uint32_t* ref, fovpt_quality_sums* out_sums, uint8_t* out_class)
{
    if (!out_sums) {
        HIPCHK(c, c->q_sums.reserve(sizeof(fovpt_quality_sums)));           // (made here, and the launch below writes every byte of it)
        out_sums = (fovpt_quality_sums*)c->q_sums.p;
    }
    HIPCHK(c, c->q_rows.reserve((size_t)fovpt_quality_rows(c->dn_w, c->dn_h) * FOVPT_QUALITY_COLUMNS * sizeof(uint64_t)));
    QualityArgs a;
    memset(&a, 0, sizeof(a));
    a.cx = (int64_t)(int32_t)c->dn_frame.cx; a.cy = (int64_t)(int32_t)c->dn_frame.cy;      // the rendered gaze
    a.flags = qc->flags; a.ring_width = qc->ring_width;
    a.uniform = c->dn_uniform != 0;
    fovpt_launch_quality(c->shadow_stream, c->dn_frame, a, test, ref, (uint64_t*)c->q_rows.p, out_sums, out_class);
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

// fovpt_temporal (motion false) and fovpt_temporal_motion (motion true)
int temporal_step(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_temporal_config* tc, const fovpt_float4* in_color,
                  fovpt_float4* out_color, uint32_t* out_rgba, fovpt_float4* out_motion, bool motion, const char* who)
{
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !tc) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    const fovpt_float4* in = in_color ? in_color : lp->frame.accum_buffer;
    { const int rc_ = temporal_check(c, lp, tc, in, who); if (rc_) return rc_; }
    HIPCHK(c, hipSetDevice(c->device));
    { const int rc_ = reserve_temporal(c, (size_t)c->dn_w * (size_t)c->dn_h); if (rc_) return rc_; }
    { const int rc_ = own_outputs(c, who, c->tp_color, c->tp_rgba, out_color, out_rgba); if (rc_) return rc_; }
    { const int rc_ = temporal_alias_check(c, in, out_color, out_rgba, out_motion, who); if (rc_) return rc_; }
    return temporal_enqueue(c, lp, tc, in, out_color, out_rgba, out_motion, motion, who);
}

}  // namespace

// fovpt_expose's state record, made (zeroed) on first use
static int reserve_expose_state(fovpt_ctx* c)
{
    if (c->ex_state.p) return FOVPT_OK;
    HIPCHK(c, c->ex_state.reserve(sizeof(ExposeState)));
    HIPCHK(c, hipMemset(c->ex_state.p, 0, sizeof(ExposeState)));
    return FOVPT_OK;
}

// steps = 0: the next AUTO step is a first step (no record yet: it will be made that way)
int expose_reset(fovpt_ctx* c, hipStream_t st)
{
    if (!c->ex_state.p) return FOVPT_OK;
    if (st) HIPCHK(c, hipMemsetAsync(c->ex_state.p, 0, sizeof(ExposeState), st));
    else HIPCHK(c, hipMemset(c->ex_state.p, 0, sizeof(ExposeState)));
    return FOVPT_OK;
}

// fovpt_focus's state record, made (zeroed) on first use
static int reserve_focus_state(fovpt_ctx* c)
{
    if (c->fc_state.p) return FOVPT_OK;
    HIPCHK(c, c->fc_state.reserve(sizeof(FocusState)));
    HIPCHK(c, hipMemset(c->fc_state.p, 0, sizeof(FocusState)));
    return FOVPT_OK;
}

// steps = 0: the next AUTO step is a first step (no record yet: it will be made that way)
int focus_reset(fovpt_ctx* c, hipStream_t st)
{
    if (!c->fc_state.p) return FOVPT_OK;
    if (st) HIPCHK(c, hipMemsetAsync(c->fc_state.p, 0, sizeof(FocusState), st));
    else HIPCHK(c, hipMemset(c->fc_state.p, 0, sizeof(FocusState)));
    return FOVPT_OK;
}

// the G-buffer's buffers for n pixels (the counters once: k_gbuffer_rays rewrites the queue sizes it uses on every call)
int reserve_gbuffer(fovpt_ctx* c, size_t n)
{
    const bool fresh = c->gb_cnt.p == nullptr;
    HIPCHK(c, c->gb_o.reserve(n * 16)); HIPCHK(c, c->gb_d.reserve(n * 16)); HIPCHK(c, c->gb_hit.reserve(n * 16));
    HIPCHK(c, c->gb_prim.reserve(n * 4)); HIPCHK(c, c->gb_pos.reserve(n * 16)); HIPCHK(c, c->gb_nrm.reserve(n * 16)); HIPCHK(c, c->gb_alb.reserve(n * 16));
    HIPCHK(c, c->gb_cnt.reserve(sizeof(Counters)));
    if (fresh) HIPCHK(c, hipMemset(c->gb_cnt.p, 0, sizeof(Counters)));
    return FOVPT_OK;
}

// fovpt_temporal's G-buffer sets, histories and outputs for n pixels
int reserve_temporal(fovpt_ctx* c, size_t n)
{
    for (int k = 0; k < 2; k++) {
        HIPCHK(c, c->tp_prim[k].reserve(n * 4)); HIPCHK(c, c->tp_pos[k].reserve(n * 16)); HIPCHK(c, c->tp_nrm[k].reserve(n * 16));
        HIPCHK(c, c->tp_alb[k].reserve(n * 16)); HIPCHK(c, c->tp_hist[k].reserve(n * 16));
    }
    HIPCHK(c, c->tp_color.reserve(n * 16)); HIPCHK(c, c->tp_rgba.reserve(n * 4));
    return FOVPT_OK;
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
    { const int rc_ = reserve_gbuffer(c, n); if (rc_) return rc_; }
    c->gb_pixels = n;
    // fovpt_warp_motion: whose hit records these are -- the rendered frame's when this is its size and camera
    if (w == c->dn_w && h == c->dn_h && !memcmp(view.eye, c->dn_frame.eye, sizeof(view.eye)) && !memcmp(view.U, c->dn_frame.U, sizeof(view.U)) &&
        !memcmp(view.V, c->dn_frame.V, sizeof(view.V)) && !memcmp(view.W, c->dn_frame.W, sizeof(view.W)))
        c->gb_stamp = ++c->seq;
    FrameDev fd;
    memset(&fd, 0, sizeof(fd));
    fd.w = w; fd.h = h;
    memcpy(fd.eye, view.eye, sizeof(fd.eye)); memcpy(fd.U, view.U, sizeof(fd.U));
    memcpy(fd.V, view.V, sizeof(fd.V)); memcpy(fd.W, view.W, sizeof(fd.W));
    RayQueue q; q.o = (float4*)c->gb_o.p; q.d = (float4*)c->gb_d.p;
    PathState ps;
    memset(&ps, 0, sizeof(ps));
    ps.hit = (float4*)c->gb_hit.p;                                   // all a closest-hit launch writes
    ShadowQueue sq;
    memset(&sq, 0, sizeof(sq));
    Counters* cnt = (Counters*)c->gb_cnt.p;
    if (target) g = *target;
    else { g.prim = (uint32_t*)c->gb_prim.p; g.pos = (float4*)c->gb_pos.p; g.nrm = (float4*)c->gb_nrm.p; g.alb = (float4*)c->gb_alb.p; }
    hipStream_t st = c->shadow_stream;
    fovpt_launch_gbuffer_rays(st, fd, q, cnt);
    fovpt_launch_traverse(st, scene_view(c), ps, q, sq, (uint32_t)n, cnt, 0, -1, c->grid_trace);   // shard 0 holds all n rays
    fovpt_launch_gbuffer_fill(st, fd, scene_view(c), q, ps.hit, g);
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

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
    if (!out) return FOVPT_E_INVALID;
    memset(out, 0, sizeof(*out));
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
    if (!c || !color || !rgba) return FOVPT_E_INVALID;
    *color = nullptr; *rgba = nullptr;
    return own_outputs(c, "fovpt_denoise_buffers", c->dn_color, c->dn_rgba, *color, *rgba);
}

// Enqueued on the stream every resolve runs on (fovpt_stream()), in issue order: behind the resolve of the frame last issued
// -- also with frames_in_flight = 2 or chains_per_frame = 2, whose chains all join that stream for their resolve -- and ahead
// of the next frame's resolve, the first of its launches that rewrites accum / frame / guides (its memsets and snapshot copies
// of chunked launches also run there).  Callers synchronising on fovpt_stream() see the denoised frame.
int fovpt_denoise(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_denoise_config* dc, fovpt_float4* out_color, uint32_t* out_rgba)
{
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !dc) return fail(c, FOVPT_E_INVALID, "fovpt_denoise: null argument");
    { const int rc_ = denoise_check(c, lp, dc, "fovpt_denoise"); if (rc_) return rc_; }
    HIPCHK(c, hipSetDevice(c->device));
    { const int rc_ = own_outputs(c, "fovpt_denoise", c->dn_color, c->dn_rgba, out_color, out_rgba); if (rc_) return rc_; }
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
    const int rc = enqueue_gbuffer(c, lp, view, g, "fovpt_gbuffer");
    if (rc) return rc;
    out->prim = g.prim;
    out->position = (fovpt_float4*)g.pos; out->normal = (fovpt_float4*)g.nrm; out->albedo = (fovpt_float4*)g.alb;
    out->width = lp->frame.size.x; out->height = lp->frame.size.y;
    return FOVPT_OK;
}

int fovpt_reconstruct_defaults(fovpt_reconstruct_config* out)
{
    if (!out) return FOVPT_E_INVALID;
    memset(out, 0, sizeof(*out));
    out->support = FOVPT_RECONSTRUCT_SUPPORT;
    out->normal_sigma = FOVPT_RECONSTRUCT_NORMAL_SIGMA;
    out->depth_sigma = FOVPT_RECONSTRUCT_DEPTH_SIGMA;
    out->levels = 3;
    out->remodulate = 1;
    return FOVPT_OK;
}

int fovpt_reconstruct_buffers(fovpt_ctx* c, fovpt_float4** color, uint32_t** rgba)
{
    if (!c || !color || !rgba) return FOVPT_E_INVALID;
    *color = nullptr; *rgba = nullptr;
    return own_outputs(c, "fovpt_reconstruct_buffers", c->rc_color, c->rc_rgba, *color, *rgba);
}

// Enqueued on fovpt_stream() like fovpt_denoise, and ordered like it: behind the resolve of the frame last issued, ahead of
// the next frame's.  Builds that frame's G-buffer first (the same stream), then reconstructs.
int fovpt_reconstruct(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_reconstruct_config* rc, const fovpt_float4* in_color,
                      fovpt_float4* out_color, uint32_t* out_rgba)
{
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !rc) return fail(c, FOVPT_E_INVALID, "fovpt_reconstruct: null argument");
    const fovpt_float4* in = in_color ? in_color : lp->frame.accum_buffer;
    { const int rc_ = reconstruct_check(c, lp, rc, in, "fovpt_reconstruct"); if (rc_) return rc_; }
    HIPCHK(c, hipSetDevice(c->device));
    { const int rc_ = own_outputs(c, "fovpt_reconstruct", c->rc_color, c->rc_rgba, out_color, out_rgba); if (rc_) return rc_; }
    if (in == out_color) return fail(c, FOVPT_E_INVALID, "fovpt_reconstruct: the input is the output colour buffer (it reads neighbours)");
    return reconstruct_enqueue(c, lp, rc, in, out_color, out_rgba, "fovpt_reconstruct");
}

// ---- temporal reprojection of the frame history (temporal.hip; its definition: tests/temporal_ref.py) ------------------
int fovpt_temporal_defaults(fovpt_temporal_config* out)
{
    if (!out) return FOVPT_E_INVALID;
    memset(out, 0, sizeof(*out));
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
    if (!c || !color || !rgba || !history) return FOVPT_E_INVALID;
    *color = nullptr; *rgba = nullptr;
    int rc_ = own_outputs(c, "fovpt_temporal_buffers", c->tp_color, c->tp_rgba, *color, *rgba);
    if (rc_ == FOVPT_OK && !c->tp_hist[0].p) rc_ = reserve_temporal(c, (size_t)c->dn_w * (size_t)c->dn_h);      // the histories and G-buffer sets with them
    if (rc_) return rc_;
    *history = (const fovpt_float4*)c->tp_hist[c->tp_last].p;
    return FOVPT_OK;
}

int fovpt_temporal_reset(fovpt_ctx* c)
{
    if (!c) return FOVPT_E_INVALID;
    c->tp_valid = false;
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
    if (!out) return FOVPT_E_INVALID;
    memset(out, 0, sizeof(*out));
    out->stages = FOVPT_POST_RECONSTRUCT | FOVPT_POST_TEMPORAL | FOVPT_POST_MOTION;
    (void)fovpt_denoise_defaults(&out->denoise);
    (void)fovpt_reconstruct_defaults(&out->reconstruct);
    (void)fovpt_temporal_defaults(&out->temporal);
    return FOVPT_OK;
}

int fovpt_post_buffers(fovpt_ctx* c, fovpt_float4** color, uint32_t** rgba)
{
    if (!c || !color || !rgba) return FOVPT_E_INVALID;
    *color = nullptr; *rgba = nullptr;
    return own_outputs(c, "fovpt_post_buffers", c->po_color, c->po_rgba, *color, *rgba);
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
    for (int32_t r : pc->_reserved)
        if (r != 0) return fail(c, FOVPT_E_INVALID, "%s: reserved fields must be 0", who);
#if FOVPT_V_STEPSTAT
    if (R || T) return fail(c, FOVPT_E_INVALID, "%s: the G-buffer is not available in a diagnostic (FOVPT_V_STEPSTAT) build", who);
#endif
    // the later stages' colour input where no stage makes it (a stage's output is never null: any non-null value stands for it)
    const fovpt_float4* in0 = in_color ? in_color : lp->frame.accum_buffer;
    const fovpt_float4* const made = (const fovpt_float4*)c;
    if (D) { const int rc_ = denoise_check(c, lp, &pc->denoise, who); if (rc_) return rc_; }
    if (R) { const int rc_ = reconstruct_check(c, lp, &pc->reconstruct, D ? made : in0, who); if (rc_) return rc_; }
    if (T) { const int rc_ = temporal_check(c, lp, &pc->temporal, D || R ? made : in0, who); if (rc_) return rc_; }

    // buffers: the denoiser's own where a stage follows it, the step's sets and histories, the call's outputs
    HIPCHK(c, hipSetDevice(c->device));
    fovpt_float4* dn_color = nullptr;
    uint32_t* dn_rgba = nullptr;
    if (D && (R || T)) { const int rc_ = own_outputs(c, who, c->dn_color, c->dn_rgba, dn_color, dn_rgba); if (rc_) return rc_; }
    if (T) { const int rc_ = reserve_temporal(c, (size_t)c->dn_w * (size_t)c->dn_h); if (rc_) return rc_; }
    { const int rc_ = own_outputs(c, who, c->po_color, c->po_rgba, out_color, out_rgba); if (rc_) return rc_; }
    const fovpt_float4* in = D ? dn_color : in0;                            // what the stage after the denoiser reads
    if (R && in == out_color) return fail(c, FOVPT_E_INVALID, "%s: the reconstruction's input is the output colour buffer (it reads neighbours)", who);
    if (T) { const int rc_ = temporal_alias_check(c, in, out_color, out_rgba, out_motion, who); if (rc_) return rc_; }
    if (R && T) {                                                          // one kernel reads `in` and the albedo guide across pixels
        const void* wr[4] = {out_rgba, out_motion, c->tp_hist[0].p, c->tp_hist[1].p};
        const void* alb = pc->reconstruct.remodulate ? (const void*)lp->frame.albedo_buffer : nullptr;
        for (const void* w : wr)
            if (w && (w == (const void*)in || w == alb)) return fail(c, FOVPT_E_INVALID, "%s: an output or history buffer is the reconstruction's input or the albedo guide", who);
        if (alb && (const void*)out_color == alb) return fail(c, FOVPT_E_INVALID, "%s: the output colour buffer is the albedo guide", who);
    }

    if (D) {
        const int rc_ = R || T ? denoise_enqueue(c, lp, &pc->denoise, dn_color, dn_rgba) : denoise_enqueue(c, lp, &pc->denoise, out_color, out_rgba);
        if (rc_) return rc_;
    }
    if (R && !T) return reconstruct_enqueue(c, lp, &pc->reconstruct, in, out_color, out_rgba, who);
    if (T) {
        ReconstructArgs ra;
        if (R) ra = reconstruct_args(&pc->reconstruct);
        return temporal_enqueue(c, lp, &pc->temporal, in, out_color, out_rgba, out_motion, M, who, R ? &ra : nullptr);
    }
    return FOVPT_OK;
}

// ---- gaze-metered auto-exposure and tone map (expose.hip; its definition: tests/expose_ref.py) ---------------------------
// (conventions, not measurements: include/fovpt.h)
int fovpt_expose_defaults(fovpt_expose_config* out)
{
    if (!out) return FOVPT_E_INVALID;
    memset(out, 0, sizeof(*out));
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
    if (!c || !color || !rgba) return FOVPT_E_INVALID;
    *color = nullptr; *rgba = nullptr;
    return own_outputs(c, "fovpt_expose_buffers", c->ex_color, c->ex_rgba, *color, *rgba);
}

int fovpt_expose_state(fovpt_ctx* c, struct fovpt_expose_state* out)
{
    if (!c) return FOVPT_E_INVALID;
    if (!out) return fail(c, FOVPT_E_INVALID, "fovpt_expose_state: null argument");
    memset(out, 0, sizeof(*out));
    if (!c->ex_state.p) return FOVPT_OK;                                   // no step yet
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->shadow_stream));
    HIPCHK(c, hipMemcpy(out, c->ex_state.p, sizeof(*out), hipMemcpyDeviceToHost));
    return FOVPT_OK;
}

int fovpt_expose_reset(fovpt_ctx* c)
{
    if (!c) return FOVPT_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    return expose_reset(c, c->shadow_stream);
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
    { const int rc_ = expose_check(c, lp, ec, in, who); if (rc_) return rc_; }
    HIPCHK(c, hipSetDevice(c->device));
    { const int rc_ = own_outputs(c, who, c->ex_color, c->ex_rgba, out_color, out_rgba); if (rc_) return rc_; }
    const size_t npix = (size_t)c->dn_w * (size_t)c->dn_h;
    const bool aut = ec->mode == FOVPT_EXPOSE_AUTO;
    const uint32_t nrows = fovpt_expose_rows(npix);
    if (aut) {
        { const int rc_ = reserve_expose_state(c); if (rc_) return rc_; }
        HIPCHK(c, c->ex_rows.reserve((size_t)nrows * FOVPT_EXPOSE_BINS * sizeof(uint32_t)));
        HIPCHK(c, c->ex_hist.reserve(FOVPT_EXPOSE_BINS * sizeof(uint64_t)));
    }
    ExposeArgs a;
    memset(&a, 0, sizeof(a));
    a.weight[0] = ec->weight_fovea; a.weight[1] = ec->weight_middle; a.weight[2] = ec->weight_periphery; a.weight[3] = ec->weight_uniform;
    a.uniform = c->dn_uniform != 0;
    a.low = ec->low_permille; a.high = ec->high_permille;
    a.ev_min = ec->ev_min; a.ev_max = ec->ev_max; a.key = ec->key;
    a.adapt_brighter = ec->adapt_brighter; a.adapt_darker = ec->adapt_darker;
    a.tone = ec->tone; a.white = ec->white; a.exposure = ec->exposure;
    const hipStream_t st = c->shadow_stream;
    if (aut) {
        fovpt_launch_expose_meter(st, c->dn_frame, a, ec->metering == FOVPT_METER_GAZE, in, (uint32_t*)c->ex_rows.p);
        fovpt_launch_expose_adapt(st, a, (const uint32_t*)c->ex_rows.p, nrows, (uint64_t*)c->ex_hist.p, (ExposeState*)c->ex_state.p);
    }
    fovpt_launch_expose_apply(st, npix, a, aut ? (const ExposeState*)c->ex_state.p : nullptr, in, out_color, out_rgba);
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

// ---- late reprojection of the finished frame to a newer camera (warp.hip; its definition: tests/warp_ref.py) ------------------
// (fill_radius: a convention, not a measurement: include/fovpt.h)
int fovpt_warp_defaults(fovpt_warp_config* out)
{
    if (!out) return FOVPT_E_INVALID;
    memset(out, 0, sizeof(*out));
    out->images = FOVPT_WARP_COLOR | FOVPT_WARP_RGBA;
    out->fill_radius = 2;
    return FOVPT_OK;
}

int fovpt_warp_buffers(fovpt_ctx* c, fovpt_float4** color, uint32_t** rgba)
{
    if (!c || !color || !rgba) return FOVPT_E_INVALID;
    *color = nullptr; *rgba = nullptr;
    return own_outputs(c, "fovpt_warp_buffers", c->wp_color, c->wp_rgba, *color, *rgba);
}

int fovpt_warp_counts(fovpt_ctx* c, struct fovpt_warp_counts* out)
{
    if (!c) return FOVPT_E_INVALID;
    if (!out) return fail(c, FOVPT_E_INVALID, "fovpt_warp_counts: null argument");
    memset(out, 0, sizeof(*out));
    if (!c->wp_counts.p) return FOVPT_OK;                                  // no warp yet
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->shadow_stream));
    std::vector<uint64_t> part(FOVPT_WARP_COUNT_BYTES / sizeof(uint64_t));
    HIPCHK(c, hipMemcpy(part.data(), c->wp_counts.p, FOVPT_WARP_COUNT_BYTES, hipMemcpyDeviceToHost));
    for (size_t s = 0; s < FOVPT_WARP_COUNT_SLOTS; s++) {                  // the waves' partial records
        const uint64_t* p = &part[s * FOVPT_WARP_COUNT_STRIDE];
        out->splatted += p[0]; out->direct += p[1]; out->filled += p[2]; out->empty += p[3];
    }
    return FOVPT_OK;
}

int fovpt_temporal_gbuffer(fovpt_ctx* c, fovpt_gbuffer_ptrs* out)
{
    if (!c) return FOVPT_E_INVALID;
    if (!out) return fail(c, FOVPT_E_INVALID, "fovpt_temporal_gbuffer: null argument");
    if (!c->tp_valid) return fail(c, FOVPT_E_NO_FRAME, "fovpt_temporal_gbuffer: no temporal step since create / reset / resize / set_scene");
    const GBufferDev g = temporal_set(c, c->tp_last);
    out->prim = g.prim;
    out->position = (fovpt_float4*)g.pos; out->normal = (fovpt_float4*)g.nrm; out->albedo = (fovpt_float4*)g.alb;
    out->width = c->tp_w; out->height = c->tp_h;
    return FOVPT_OK;
}

// What fovpt_warp and fovpt_warp_motion (`who`) share.  A checked call: the scatter's camera, the enabled images and their inputs,
// the G-buffer the scatter reads.
struct WarpCall {
    WarpArgs a;
    size_t npix;
    bool C_, R_;
    const fovpt_float4* in;
    const uint32_t* rin;
    GBufferDev g;
};

// the validation up to the inputs, in fovpt_warp's order (nothing allocated, enqueued or changed).  reserved: the config's nres words
static int warp_check(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_warp_camera* to, int32_t images, int32_t fill_radius, const int32_t* reserved,
                      int nres, const fovpt_gbuffer_ptrs* gbuffer, const fovpt_float4* in_color, const uint32_t* in_rgba, const char* who, WarpCall& w)
{
    if (images == 0 || (images & ~(FOVPT_WARP_COLOR | FOVPT_WARP_RGBA)))
        return fail(c, FOVPT_E_INVALID, "%s: images %d names no image or an unknown one", who, images);
    if (fill_radius < 0 || fill_radius > FOVPT_WARP_MAX_RADIUS)
        return fail(c, FOVPT_E_INVALID, "%s: fill_radius %d outside 0 .. %d", who, fill_radius, FOVPT_WARP_MAX_RADIUS);
    for (int k = 0; k < nres; k++)
        if (reserved[k] != 0) return fail(c, FOVPT_E_INVALID, "%s: reserved fields must be 0", who);
    const float* cam = &to->eye.x;                                         // eye, U, V, W: 12 floats
    for (int k = 0; k < 12; k++)
        if (!std::isfinite(cam[k])) return fail(c, FOVPT_E_INVALID, "%s: the camera to warp to has a non-finite entry", who);
    memset(&w.a, 0, sizeof(w.a));
    if (!camera_inverse(&to->U.x, &to->V.x, &to->W.x, w.a.inv)) return fail(c, FOVPT_E_INVALID, "%s: the camera to warp to is singular", who);
    memcpy(w.a.eye, &to->eye.x, sizeof(w.a.eye));
    if (!gbuffer && (!c->has_scene || lp->traversable != c->scene_id)) return fail(c, FOVPT_E_NO_SCENE, "%s without a scene", who);
    { const int rc_ = check_rendered_frame(c, lp, who, "warp", nullptr); if (rc_) return rc_; }
    w.npix = (size_t)c->dn_w * (size_t)c->dn_h;
    if (w.npix >= (1ull << 30)) return fail(c, FOVPT_E_INVALID, "%s: frame too large (%d x %d)", who, c->dn_w, c->dn_h);
    if (gbuffer && (gbuffer->width != c->dn_w || gbuffer->height != c->dn_h || !gbuffer->prim || !gbuffer->position))
        return fail(c, FOVPT_E_INVALID, "%s: the G-buffer is not of the frame's size %d x %d, or has a null prim or position", who, c->dn_w, c->dn_h);
    w.C_ = images & FOVPT_WARP_COLOR; w.R_ = images & FOVPT_WARP_RGBA;
    w.in = w.C_ ? (in_color ? in_color : lp->frame.accum_buffer) : nullptr;
    w.rin = w.R_ ? (in_rgba ? in_rgba : lp->frame.frame_buffer) : nullptr;
    if ((w.C_ && !w.in) || (w.R_ && !w.rin)) return fail(c, FOVPT_E_INVALID, "%s: an enabled image has a null input", who);
    return FOVPT_OK;
}

// the buffers of a checked call -- the context's own outputs where an enabled image has none, the keys, the counts -- and the last
// of the validation, which needs them: no output is an input, the keys or another output (the resolve reads other pixels' inputs
// and keys while it writes)
static int warp_buffers(fovpt_ctx* c, const fovpt_gbuffer_ptrs* gbuffer, WarpCall& w, fovpt_float4*& out_color, uint32_t*& out_rgba, uint32_t* out_map,
                        const char* who)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (w.C_ && !out_color) { HIPCHK(c, c->wp_color.reserve(w.npix * 16)); out_color = (fovpt_float4*)c->wp_color.p; }
    if (w.R_ && !out_rgba) { HIPCHK(c, c->wp_rgba.reserve(w.npix * 4)); out_rgba = (uint32_t*)c->wp_rgba.p; }
    if (!w.C_) out_color = nullptr;
    if (!w.R_) out_rgba = nullptr;
    HIPCHK(c, c->wp_keys.reserve(w.npix * 8));
    if (!c->wp_counts.p) {
        HIPCHK(c, c->wp_counts.reserve(FOVPT_WARP_COUNT_BYTES));
        HIPCHK(c, hipMemset(c->wp_counts.p, 0, FOVPT_WARP_COUNT_BYTES));
    }
    GBufferDev& g = w.g;
    if (gbuffer) { g.prim = gbuffer->prim; g.pos = (float4*)gbuffer->position; g.nrm = (float4*)gbuffer->normal; g.alb = (float4*)gbuffer->albedo; }
    else { g.prim = (uint32_t*)c->gb_prim.p; g.pos = (float4*)c->gb_pos.p; g.nrm = nullptr; g.alb = nullptr; }      // (null until the first trace)
    const void* outs[3] = {out_color, out_rgba, out_map};
    const void* ins[5] = {w.in, w.rin, g.prim, g.pos, c->wp_keys.p};
    for (int i = 0; i < 3; i++) {
        if (!outs[i]) continue;
        for (const void* p : ins)
            if (p == outs[i]) return fail(c, FOVPT_E_INVALID, "%s: an output is an input of the call (the resolve reads across pixels)", who);
        for (int j = 0; j < i; j++)
            if (outs[j] == outs[i]) return fail(c, FOVPT_E_INVALID, "%s: two outputs are the same buffer", who);
    }
    return FOVPT_OK;
}

// Enqueued on fovpt_stream() like fovpt_denoise, and ordered like it.  Without a caller's G-buffer the rendered frame's first (the
// same stream, into fovpt_gbuffer's buffers); then the keys and counts are cleared, k_warp_scatter (motion null) or
// k_warp_scatter_motion (motion: its advance; the rest is filled in here, behind the trace), k_warp_resolve.
static int warp_enqueue(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_gbuffer_ptrs* gbuffer, WarpCall& w, int32_t fill_radius,
                        const float* motion, fovpt_float4* out_color, uint32_t* out_rgba, uint32_t* out_map, const char* who)
{
    if (!gbuffer) { const int rc_ = enqueue_gbuffer(c, lp, c->dn_frame, w.g, who); if (rc_) return rc_; }   // the rendered frame's camera
    const hipStream_t st = c->shadow_stream;
    HIPCHK(c, hipMemsetAsync(c->wp_keys.p, 0xff, w.npix * 8, st));
    HIPCHK(c, hipMemsetAsync(c->wp_counts.p, 0, FOVPT_WARP_COUNT_BYTES, st));
    if (!motion) fovpt_launch_warp_scatter(st, c->dn_frame, w.a, w.g.prim, w.g.pos, (uint64_t*)c->wp_keys.p, (uint64_t*)c->wp_counts.p);
    else {
        WarpMotionArgs m;
        memset(&m, 0, sizeof(m));
        m.hit = (const float4*)c->gb_hit.p; m.tris = c->tris;
        m.mark = (const uint64_t*)c->tm_mark.p; m.epoch = c->tm_epoch - 1;     // the step that ended the last interval
        m.tri_vidx = (const uint3*)c->up_vidx.p; m.vtx_prev = (const float*)c->vtx_prev.p;
        m.tri_bytes = (uint64_t)c->num_tris * sizeof(TriRec);
        m.num_prims = (uint32_t)(c->h_tri_vidx.size() / 3); m.num_meshes = (uint32_t)c->mesh_nv.size();
        m.advance = *motion;
        fovpt_launch_warp_scatter_motion(st, c->dn_frame, w.a, m, w.g.prim, w.g.pos, (uint64_t*)c->wp_keys.p, (uint64_t*)c->wp_counts.p);
    }
    fovpt_launch_warp_resolve(st, c->dn_w, c->dn_h, fill_radius, (const uint64_t*)c->wp_keys.p, w.in, w.rin, out_color, out_rgba, out_map,
                              (uint64_t*)c->wp_counts.p);
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

int fovpt_warp(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_warp_camera* to, const fovpt_warp_config* wc, const fovpt_gbuffer_ptrs* gbuffer,
               const fovpt_float4* in_color, const uint32_t* in_rgba, fovpt_float4* out_color, uint32_t* out_rgba, uint32_t* out_map)
{
    const char* who = "fovpt_warp";
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !to || !wc) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    WarpCall w;
    { const int rc_ = warp_check(c, lp, to, wc->images, wc->fill_radius, wc->_reserved, 6, gbuffer, in_color, in_rgba, who, w); if (rc_) return rc_; }
    { const int rc_ = warp_buffers(c, gbuffer, w, out_color, out_rgba, out_map, who); if (rc_) return rc_; }
    return warp_enqueue(c, lp, gbuffer, w, wc->fill_radius, nullptr, out_color, out_rgba, out_map, who);
}

// ---- fovpt_warp in which the meshes that moved in the last interval go on moving (warp.hip, k_warp_scatter_motion; its definition:
// tests/warp_motion_ref.py) ----------------------------------------------------------------------------
// (advance: a convention, not a measurement: include/fovpt.h)
int fovpt_warp_motion_defaults(fovpt_warp_motion_config* out)
{
    if (!out) return FOVPT_E_INVALID;
    memset(out, 0, sizeof(*out));
    out->images = FOVPT_WARP_COLOR | FOVPT_WARP_RGBA;
    out->fill_radius = 2;
    out->advance = 1.0f;
    return FOVPT_OK;
}

int fovpt_warp_motion(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_warp_camera* to, const fovpt_warp_motion_config* mc,
                      const fovpt_gbuffer_ptrs* gbuffer, const fovpt_float4* in_color, const uint32_t* in_rgba, fovpt_float4* out_color,
                      uint32_t* out_rgba, uint32_t* out_map)
{
    const char* who = "fovpt_warp_motion";
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !to || !mc) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    if (!(mc->advance >= 0.0f && mc->advance <= FOVPT_WARP_MAX_ADVANCE))   // (NaN fails)
        return fail(c, FOVPT_E_INVALID, "%s: advance %g outside 0 .. %g", who, (double)mc->advance, (double)FOVPT_WARP_MAX_ADVANCE);
    WarpCall w;
    { const int rc_ = warp_check(c, lp, to, mc->images, mc->fill_radius, mc->_reserved, 5, gbuffer, in_color, in_rgba, who, w); if (rc_) return rc_; }
    // the last temporal step, the previous positions and the hit records describe the rendered frame
    if (!c->tp_valid) return fail(c, FOVPT_E_NO_FRAME, "%s: no temporal step since create / reset / resize / set_scene", who);
    if (!c->tm_tracking)
        return fail(c, FOVPT_E_NO_FRAME, "%s: previous positions are not tracked yet (no fovpt_temporal_motion or fovpt_post with MOTION on this scene)", who);
    if (c->seq_update > c->seq_step)
        return fail(c, FOVPT_E_NO_FRAME, "%s: a geometry update has been issued since the last temporal step", who);
    if (gbuffer && !(c->gb_stamp > c->seq_frame && c->gb_stamp > c->seq_update && c->gb_stamp > c->seq_adopt))
        return fail(c, FOVPT_E_NO_FRAME, "%s: the context's last G-buffer trace is not of the rendered frame and the current geometry "
                                         "(its hit records go with the caller's G-buffer)", who);
    { const int rc_ = warp_buffers(c, gbuffer, w, out_color, out_rgba, out_map, who); if (rc_) return rc_; }
    // what the host knows: with no mesh moved in the interval, a step that did not see its updates, or no advance, fovpt_warp's scatter
    bool moved = false;
    if (!c->tm_step_blind && mc->advance != 0.0f)
        for (const uint64_t e : c->tm_mesh_epoch) moved = moved || e == c->tm_epoch - 1;
    return warp_enqueue(c, lp, gbuffer, w, mc->fill_radius, moved ? &mc->advance : nullptr, out_color, out_rgba, out_map, who);
}

// ---- gaze-metered focus distance and depth of field (focus.hip; its definition: tests/focus_ref.py) ---------------------------
// (conventions, not measurements: include/fovpt.h)
int fovpt_focus_defaults(fovpt_focus_config* out)
{
    if (!out) return FOVPT_E_INVALID;
    memset(out, 0, sizeof(*out));
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
    if (!c || !color || !rgba) return FOVPT_E_INVALID;
    *color = nullptr; *rgba = nullptr;
    return own_outputs(c, "fovpt_focus_buffers", c->fc_color, c->fc_rgba, *color, *rgba);
}

int fovpt_focus_state(fovpt_ctx* c, struct fovpt_focus_state* out)
{
    if (!c) return FOVPT_E_INVALID;
    if (!out) return fail(c, FOVPT_E_INVALID, "fovpt_focus_state: null argument");
    memset(out, 0, sizeof(*out));
    if (!c->fc_state.p) return FOVPT_OK;                                   // no AUTO step yet
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->shadow_stream));
    HIPCHK(c, hipMemcpy(out, c->fc_state.p, sizeof(*out), hipMemcpyDeviceToHost));
    return FOVPT_OK;
}

int fovpt_focus_reset(fovpt_ctx* c)
{
    if (!c) return FOVPT_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    return focus_reset(c, c->shadow_stream);
}

// Enqueued on fovpt_stream() like fovpt_denoise, and ordered like it.  Without a caller's G-buffer the rendered frame's first (the
// same stream, into fovpt_gbuffer's buffers).  AUTO: k_focus_meter, k_focus_radius, k_focus_gather; the focus goes from the first to
// the second through the state record, never through the host.  FIXED: the last two.
int fovpt_focus(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_focus_config* fc, const fovpt_gbuffer_ptrs* gbuffer,
                const fovpt_float4* in_color, fovpt_float4* out_color, uint32_t* out_rgba, float* out_coc)
{
    const char* who = "fovpt_focus";
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !fc) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
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
    for (int32_t r : fc->_reserved)
        if (r != 0) return fail(c, FOVPT_E_INVALID, "%s: reserved fields must be 0", who);
    if (!gbuffer && (!c->has_scene || lp->traversable != c->scene_id)) return fail(c, FOVPT_E_NO_SCENE, "%s without a scene", who);
    { const int rc_ = check_rendered_frame(c, lp, who, "gather from", nullptr); if (rc_) return rc_; }
    const size_t npix = (size_t)c->dn_w * (size_t)c->dn_h;
    if (npix >= (1ull << 31)) return fail(c, FOVPT_E_INVALID, "%s: frame too large (%d x %d)", who, c->dn_w, c->dn_h);
    if (gbuffer && (gbuffer->width != c->dn_w || gbuffer->height != c->dn_h || !gbuffer->prim || !gbuffer->position))
        return fail(c, FOVPT_E_INVALID, "%s: the G-buffer is not of the frame's size %d x %d, or has a null prim or position", who, c->dn_w, c->dn_h);
    const fovpt_float4* in = in_color ? in_color : lp->frame.accum_buffer;
    if (!in) return fail(c, FOVPT_E_INVALID, "%s: null accum_buffer", who);

    // buffers: the context's own outputs where the caller gave none, the (r, tp) pairs, the state
    HIPCHK(c, hipSetDevice(c->device));
    { const int rc_ = own_outputs(c, who, c->fc_color, c->fc_rgba, out_color, out_rgba); if (rc_) return rc_; }
    HIPCHK(c, c->fc_rt.reserve(npix * 8));
    const bool aut = fc->mode == FOVPT_FOCUS_AUTO;
    if (aut) { const int rc_ = reserve_focus_state(c); if (rc_) return rc_; }
    // the gather reads other pixels' colours and pairs while it writes, the radius pass the G-buffer: no output is one of them
    GBufferDev g;
    if (gbuffer) { g.prim = gbuffer->prim; g.pos = (float4*)gbuffer->position; g.nrm = (float4*)gbuffer->normal; g.alb = (float4*)gbuffer->albedo; }
    else { g.prim = (uint32_t*)c->gb_prim.p; g.pos = (float4*)c->gb_pos.p; g.nrm = nullptr; g.alb = nullptr; }      // (null until the first trace)
    const void* outs[3] = {out_color, out_rgba, out_coc};
    const void* ins[4] = {in, g.prim, g.pos, c->fc_rt.p};
    for (int i = 0; i < 3; i++) {
        if (!outs[i]) continue;
        for (const void* p : ins)
            if (p == outs[i]) return fail(c, FOVPT_E_INVALID, "%s: an output is an input of the call (the gather reads across pixels)", who);
        for (int j = 0; j < i; j++)
            if (outs[j] == outs[i]) return fail(c, FOVPT_E_INVALID, "%s: two outputs are the same buffer", who);
    }

    if (!gbuffer) { const int rc_ = enqueue_gbuffer(c, lp, c->dn_frame, g, who); if (rc_) return rc_; }   // the rendered frame's camera
    FocusArgs a;
    memset(&a, 0, sizeof(a));
    a.cx = (int64_t)c->dn_frame.cx; a.cy = (int64_t)c->dn_frame.cy;       // (frame.c is unsigned: no difference below wraps)
    const int64_t R = fc->meter_radius;
    const int64_t x0 = a.cx - R > 0 ? a.cx - R : 0, x1 = a.cx + R < c->dn_w - 1 ? a.cx + R : c->dn_w - 1;
    const int64_t y0 = a.cy - R > 0 ? a.cy - R : 0, y1 = a.cy + R < c->dn_h - 1 ? a.cy + R : c->dn_h - 1;
    if (x0 <= x1 && y0 <= y1) { a.x0 = (int32_t)x0; a.x1 = (int32_t)x1; a.y0 = (int32_t)y0; a.y1 = (int32_t)y1; }
    else { a.x0 = a.y0 = 0; a.x1 = a.y1 = -1; }                            // the disc's square misses the frame
    a.meter_radius = fc->meter_radius; a.rank_permille = fc->rank_permille; a.max_radius = fc->max_radius;
    a.strength = fc->strength; a.focus_default = fc->focus_default;
    a.adapt_nearer = fc->adapt_nearer; a.adapt_farther = fc->adapt_farther;
    a.inv_focus = 1.0f / fc->focus_distance;
    const hipStream_t st = c->shadow_stream;
    FocusState* state = aut ? (FocusState*)c->fc_state.p : nullptr;
    if (aut) fovpt_launch_focus_meter(st, c->dn_w, a, g.prim, g.pos, state);
    fovpt_launch_focus_radius(st, npix, a, state, g.prim, g.pos, (float2*)c->fc_rt.p, out_coc);
    fovpt_launch_focus_gather(st, c->dn_w, c->dn_h, fc->max_radius, in, (const float2*)c->fc_rt.p, out_color, out_rgba);
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

// ---- head-mounted display lens pre-distortion (lens.hip; its definition: tests/lens_ref.py) ---------------------------------------
// (conventions, not measurements: include/fovpt.h)
int fovpt_lens_defaults(fovpt_lens_config* out)
{
    if (!out) return FOVPT_E_INVALID;
    memset(out, 0, sizeof(*out));
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
    if (!c || !color || !rgba) return FOVPT_E_INVALID;
    *color = nullptr; *rgba = nullptr;
    return own_outputs(c, "fovpt_lens_buffers", c->ln_color, c->ln_rgba, *color, *rgba);
}

// Enqueued on fovpt_stream() like fovpt_denoise, and ordered like it: one launch of k_lens.
int fovpt_lens(fovpt_ctx* c, const fovpt_launch_params* lp, const fovpt_lens_config* lc, const fovpt_warp_camera* to, const fovpt_float4* in_color,
               fovpt_float4* out_color, uint32_t* out_rgba)
{
    const char* who = "fovpt_lens";
    if (!c) return FOVPT_E_INVALID;
    if (!lp || !lc) return fail(c, FOVPT_E_INVALID, "%s: null argument", who);
    if (lc->filter != FOVPT_LENS_NEAREST && lc->filter != FOVPT_LENS_BILINEAR && lc->filter != FOVPT_LENS_BICUBIC)
        return fail(c, FOVPT_E_INVALID, "%s: unknown filter %d", who, lc->filter);
    if (lc->encode != FOVPT_LENS_ENCODE_DISPLAY && lc->encode != FOVPT_LENS_ENCODE_RESOLVE) return fail(c, FOVPT_E_INVALID, "%s: unknown encode %d", who, lc->encode);
    for (int32_t r : lc->_reserved0)
        if (r != 0) return fail(c, FOVPT_E_INVALID, "%s: reserved fields must be 0", who);
    for (int32_t r : lc->_reserved)
        if (r != 0) return fail(c, FOVPT_E_INVALID, "%s: reserved fields must be 0", who);
    const float fields[19] = {lc->center[0], lc->center[1], lc->scale[0], lc->scale[1], lc->k[0], lc->k[1], lc->k[2], lc->k[3], lc->chroma[0], lc->chroma[1],
                              lc->chroma[2], lc->src_center[0], lc->src_center[1], lc->src_scale[0], lc->src_scale[1], lc->border[0], lc->border[1],
                              lc->border[2], lc->border[3]};
    for (float v : fields)
        if (!std::isfinite(v)) return fail(c, FOVPT_E_INVALID, "%s: a non-finite center, scale, k, chroma, src_* or border entry", who);
    if (!(lc->clip_r2 > 0.0f)) return fail(c, FOVPT_E_INVALID, "%s: clip_r2 %g is not above 0", who, (double)lc->clip_r2);
    if (to) {
        const float* cam = &to->eye.x;                                     // eye, U, V, W: 12 floats
        for (int k = 0; k < 12; k++)
            if (!std::isfinite(cam[k])) return fail(c, FOVPT_E_INVALID, "%s: the camera to re-aim at has a non-finite entry", who);
    }
    { const int rc_ = check_rendered_frame(c, lp, who, "resample", nullptr); if (rc_) return rc_; }
    const size_t npix = (size_t)c->dn_w * (size_t)c->dn_h;
    if (npix >= (1ull << 31)) return fail(c, FOVPT_E_INVALID, "%s: frame too large (%d x %d)", who, c->dn_w, c->dn_h);
    LensArgs a;
    memset(&a, 0, sizeof(a));
    if (to) {                                                              // H = M [U_to V_to W_to], M of the rendered camera
        float M[9];
        if (!camera_inverse(c->dn_frame.U, c->dn_frame.V, c->dn_frame.W, M)) return fail(c, FOVPT_E_INVALID, "%s: the rendered camera is singular", who);
        const float* B[3] = {&to->U.x, &to->V.x, &to->W.x};               // the columns
        for (int k = 0; k < 3; k++)
            for (int j = 0; j < 3; j++)
                a.H[3 * k + j] = (float)(((double)M[3 * k] * (double)B[j][0] + (double)M[3 * k + 1] * (double)B[j][1]) + (double)M[3 * k + 2] * (double)B[j][2]);
        a.reaim = 1;
    }
    const fovpt_float4* in = in_color ? in_color : lp->frame.accum_buffer;
    if (!in) return fail(c, FOVPT_E_INVALID, "%s: null accum_buffer", who);

    HIPCHK(c, hipSetDevice(c->device));
    { const int rc_ = own_outputs(c, who, c->ln_color, c->ln_rgba, out_color, out_rgba); if (rc_) return rc_; }
    if ((const void*)out_color == (const void*)in || (const void*)out_rgba == (const void*)in)
        return fail(c, FOVPT_E_INVALID, "%s: an output is the input of the call (the gather reads across pixels)", who);
    if ((const void*)out_color == (const void*)out_rgba) return fail(c, FOVPT_E_INVALID, "%s: two outputs are the same buffer", who);

    a.filter = lc->filter; a.encode = lc->encode;
    a.mono = memcmp(&lc->chroma[0], &lc->chroma[1], 4) == 0 && memcmp(&lc->chroma[0], &lc->chroma[2], 4) == 0;
    memcpy(a.center, lc->center, sizeof(a.center)); memcpy(a.scale, lc->scale, sizeof(a.scale));
    memcpy(a.k, lc->k, sizeof(a.k)); memcpy(a.chroma, lc->chroma, sizeof(a.chroma));
    a.clip_r2 = lc->clip_r2;
    memcpy(a.src_center, lc->src_center, sizeof(a.src_center)); memcpy(a.src_scale, lc->src_scale, sizeof(a.src_scale));
    memcpy(a.border, lc->border, sizeof(a.border));
    fovpt_launch_lens(c->shadow_stream, c->dn_w, c->dn_h, a, in, out_color, out_rgba);
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

// ---- image quality of the rendered frame (quality.hip; its definition: tests/quality_ref.py) -----------------------------------
// (ring_width: a convention, not a measurement: include/fovpt.h)
int fovpt_quality_defaults(fovpt_quality_config* out)
{
    if (!out) return FOVPT_E_INVALID;
    memset(out, 0, sizeof(*out));
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
    { const int rc_ = quality_check(c, lp, qc, test, ref_rgba, who); if (rc_) return rc_; }
    HIPCHK(c, hipSetDevice(c->device));
    return quality_enqueue(c, qc, test, ref_rgba, out_sums, out_class);
}

int fovpt_quality_read(fovpt_ctx* c, fovpt_quality_sums* out)
{
    if (!c) return FOVPT_E_INVALID;
    if (!out) return fail(c, FOVPT_E_INVALID, "fovpt_quality_read: null argument");
    memset(out, 0, sizeof(*out));
    if (!c->q_sums.p) return FOVPT_OK;                                     // no measurement into the context's record yet
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->shadow_stream));
    HIPCHK(c, hipMemcpy(out, c->q_sums.p, sizeof(*out), hipMemcpyDeviceToHost));
    return FOVPT_OK;
}

}  // extern "C"
