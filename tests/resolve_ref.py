"""The resolve of a frame, restated in numpy binary32 from the reference's raygen tail (deviceProgram.cu:522-616, with the
accumulate blend of PT_sv4_vmv2/deviceProgram.cu:545-553) and SampleRenderer::render() (SimplePathtracer.cpp:77-214): what
k_resolve (csrc/wavefront.hip) must leave in the frame buffers for a given path state.

It PAINTS, as the reference does: the passes in launch order (P, M, F), within a pass the launch indices in ascending (y, x),
every launch index that passes the ring test writes its fillSize x fillSize block with the pixel indices clamped onto the
frame -- a later writer overwrites an earlier one.  There is no search for a pixel's last writer here, so it shares nothing
with find_last_writer (csrc/fovpt_pixel.h), which the kernel uses.

The path state is the library's (include/fovpt.h, fovpt_debug_resolve), in slot order: sample slot of (pass, launch index
li = ly * gw + lx, sample s) = slot_base + li * spp + s; launch record = launch_base + li.
  state = flags | depth << 8.  The path counted depth segments; cell dd of the slot holds prd.radiance of segment dd.  Only
      min(depth, max_depth) cells count (:515 discards the segment at max_depth), cell 0 is directLight (:523), the others are
      added to indirectLight in order (:526), and the sample adds directLight + indirectLight (:536).
  alpha: prd.alpha of the sample (:537) is (1, 1, 1) under ALPHA_ONE (:689), else alpha[slot] under ALPHA_SET (:693), else 0.
  guide_n / guide_a: prd.normal / prd.albedo of the sample's primary hit (:509-512), summed and divided like alpha (:541-543).
  backplate: per launch record, the backplate of the launch index's last sample (:495).

A frame sharded over `world` ranks (fovpt_config.rank / world / tile_w / tile_h, include/fovpt.h): launch index (lx, ly) of
pass p belongs to rank (lx // tile_w + 3 * (ly // tile_h) + p) % world.  A rank writes the pixels whose last writer is its
own, zeroes (float4 0, rgba 0) the pixels whose last writer is another rank's, and leaves the pixels nobody writes alone --
except on a rank other than 0 rendering a whole frame (render()), which zeroes those too, so that the ranks' frames sum to
the single-GPU frame."""
import numpy as np

f32 = np.float32
M32 = 0xffffffff
DONE, SECONDARY, ALPHA_ONE, ALPHA_SET = 1, 2, 4, 8


class Pass:
    """One optixLaunch: grid, frame.factor / fillSize / offset / r_inner / r_outer / subframe_index / redraw, samples_per_launch."""

    def __init__(self, gw, gh, factor, fill, off, r_inner, r_outer, spp, subframe, redraw):
        self.gw, self.gh, self.fx, self.fy, self.fill = int(gw), int(gh), int(factor[0]), int(factor[1]), int(fill)
        self.offx, self.offy = int(off[0]) & M32, int(off[1]) & M32
        self.r_inner, self.r_outer = f32(r_inner), f32(r_outer)
        self.spp, self.subframe, self.redraw = int(spp), int(subframe), int(redraw)
        self.slot_base = self.launch_base = 0

    def alive(self, lx, ly, gaze):
        """The ring test on the block's first pixel, :433-440 (uint32 index arithmetic)."""
        ix, iy = (lx * self.fx + self.offx) & M32, (ly * self.fy + self.offy) & M32
        dx, dy, dz = f32(ix) - f32(gaze[0]), f32(iy) - f32(gaze[1]), f32(0.0) - f32(0.0)
        rng = np.sqrt((dx * dx + dy * dy) + dz * dz)
        return not (rng < self.r_inner or rng > self.r_outer)


def launch_pass(lp, width, height):
    """The one pass of fovpt_launch(lp, width, height)."""
    f = lp.frame
    return [Pass(width, height, (f.factor.x, f.factor.y), f.fillSize, (f.offset.x, f.offset.y), f.r_inner, f.r_outer,
                 lp.samples_per_launch, f.subframe_index, f.redraw)]


def render_passes(cfg, lp):
    """The launches of SampleRenderer::render(), SimplePathtracer.cpp:85-209."""
    f = lp.frame
    w, h, cx, cy = f.size.x, f.size.y, f.c.x, f.c.y
    if cfg.uniform:                                                                    # FOV_OFF :85-131
        return [Pass(w, h, (1, 1), 1, (0, 0), 0.0, 1e9, cfg.spp_uniform, 0, 0)]
    m, fo = cfg.r_outer + 2, cfg.r_inner + 1
    return [Pass(w // 4, h // 4, (4, 4), 4, (0, 0), float(cfg.r_outer), 1e9, cfg.spp_periphery, f.subframe_index, 0),   # :137-157
            Pass(m, m, (2, 2), 2, (cx - m, cy - m), float(cfg.r_inner), float(m), cfg.spp_middle, 0, 1),               # :160-187
            Pass(2 * fo, 2 * fo, (1, 1), 1, (cx - fo, cy - fo), 0.0, float(fo), cfg.spp_fovea, 0, 1)]                 # :189-209


def layout(passes):
    """Gives every pass its place in the arrays -> (sample slots, launch records)."""
    slots = launches = 0
    for p in passes:
        p.slot_base, p.launch_base = slots, launches
        slots += p.gw * p.gh * p.spp
        launches += p.gw * p.gh
    return slots, launches


def _launch_index(P, li, max_depth, state, cells, alpha, backplate, guide_n, guide_a):
    """-> (accum_color before the blend, normal, albedo) of one launch index, :446-560."""
    z = np.zeros(3, f32)
    result, a_sum, n_sum, al_sum = z.copy(), z.copy(), z.copy(), z.copy()
    for s in range(P.spp):
        slot = P.slot_base + li * P.spp + s
        st = int(state[slot])
        nseg = min(st >> 8, max_depth)
        direct, indirect = z.copy(), z.copy()
        if nseg > 0:
            direct = direct + cells[slot, 0, :3]                                       # :523
        for dd in range(1, nseg):
            indirect = indirect + cells[slot, dd, :3]                                  # :526
        result = result + (direct + indirect)                                          # :536
        if st & ALPHA_ONE:
            a_sum = a_sum + f32(1.0)
        elif st & ALPHA_SET:
            a_sum = a_sum + alpha[slot, :3]
        else:
            a_sum = a_sum + f32(0.0)
        if guide_n is not None:
            n_sum = n_sum + guide_n[slot, :3]                                          # :510-511
            al_sum = al_sum + guide_a[slot, :3]
    sppf = f32(P.spp)
    inv = f32(1.0) / sppf                                                              # float3 /= float: times 1 / s
    n_sum, al_sum, a_sum = n_sum * inv, al_sum * inv, a_sum * inv                      # :541-543
    color = (backplate[P.launch_base + li, :3] * sppf) * (f32(1.0) - a_sum) + result   # :558
    return color * inv, n_sum, al_sum                                                  # :560


def resolve(passes, gaze, max_depth, accumulate, state, cells, alpha, backplate, bufs, make_color, guide_n=None, guide_a=None,
            rank=0, world=1, tile=(8, 4), whole_frame=False):
    """Paints bufs["accum"] (h, w, 4), bufs["frame"] (h, w) uint32 and -- with guides -- bufs["normal" / "color" / "albedo"] in
    place.  make_color: (n, 3) float32 accum colours -> rgba8 (the oracle's exposure, Reinhard and make_color, :586-597).
    Returns the (h, w) map of the pass that wrote each pixel last (-1: nobody)."""
    accum, frame = bufs["accum"], bufs["frame"]
    h, w = frame.shape
    last_pass = np.full((h, w), -1, np.int32)
    foreign = np.zeros((h, w), bool)
    untouched = {k: bufs[k].copy() for k in ("normal", "color", "albedo")} if guide_n is not None else {}
    with np.errstate(all="ignore"):
        for p, P in enumerate(passes):
            before = accum.copy()                                   # what a launch's writers blend with: the frame before it
            for ly in range(P.gh):
                for lx in range(P.gw):
                    if not P.alive(lx, ly, gaze):
                        continue
                    mine = world <= 1 or (lx // tile[0] + 3 * (ly // tile[1]) + p) % world == rank
                    if mine:
                        c, gn, ga = _launch_index(P, ly * P.gw + lx, max_depth, state, cells, alpha, backplate, guide_n, guide_a)
                    for fi in range(P.fill):                                           # :546-554
                        for fj in range(P.fill):
                            ix = min((lx * P.fx + fi + P.offx) & M32, w - 1)
                            iy = min((ly * P.fy + fj + P.offy) & M32, h - 1)
                            last_pass[iy, ix] = p
                            foreign[iy, ix] = not mine
                            if not mine:
                                for k, v in untouched.items():                         # (another rank's pixel gets no guides here)
                                    bufs[k][iy, ix] = v[iy, ix]
                                continue
                            a = c
                            if accumulate and P.subframe > 0 and not P.redraw:         # PT_sv4_vmv2 :545-553
                                a = np.fmax(f32(0.0), np.fmin(c, f32(10.0)))
                                av = f32(1.0) / f32(P.subframe + 1)
                                prev = before[iy, ix, :3]
                                a = prev + av * (a - prev)
                            accum[iy, ix, :3] = a                                      # :582
                            accum[iy, ix, 3] = f32(1.0)
                            if guide_n is not None:                                    # :612-614
                                bufs["normal"][iy, ix] = (gn[0], gn[1], gn[2], 1.0)
                                bufs["color"][iy, ix] = (a[0], a[1], a[2], 1.0)
                                bufs["albedo"][iy, ix] = (ga[0], ga[1], ga[2], 1.0)
    own = (last_pass >= 0) & ~foreign
    if own.any():
        frame[own] = make_color(accum[own][:, :3])                                     # :586-597
    zero = foreign.copy()
    if whole_frame and world > 1 and rank != 0:
        zero |= last_pass < 0
    accum[zero] = 0.0
    frame[zero] = 0
    return last_pass
