"""What k_shade (csrc/wavefront.hip) must leave for a hit, from the reference's view of it: the oracle runs traceRadiance from
just behind trace_closest twice per hit (oracle.shade_hit), once with the next-event occlusion ray unoccluded and once
occluded, and expected() maps the two RadiancePRDs onto the library's state.  The rules, each from the reference lines the
kernel's comments cite (deviceProgram.cu):

  The reference's loop around traceRadiance (:497-531): a segment whose prd comes back DONE, or at depth >= max_depth, ends
  the path and adds nothing (:515) -- except, with FOVPT_OPT_SKY_MISS, the sky term of an escaped secondary ray at
  depth < max_depth --; otherwise prd.radiance is the depth-th term (:522-527), depth goes up (:529) and the path goes on
  from prd.origin along prd.direction -- unless FOVPT_OPT_RUSSIAN_ROULETTE ended it.

  Flags and depth.  DONE follows prd.stateFlags, and is also set where the reference shades the segment it discards
  (a hit at depth >= max_depth, :515); SECONDARY follows prd.stateFlags.  ALPHA_ONE: the hit ran prd.alpha = 1 (:689, any
  shaded hit off a shadow catcher -- also a discarded one, and one whose BSDF sample failed); ALPHA_SET: the hit ran
  prd.alpha += ... (:693, a shaded hit on a catcher).  A catcher hit of a secondary ray passes through (:646-651): flags
  and depth unchanged.  A counted segment -- the sky term included -- makes depth one more.

  Radiance cell or shadow record.  The value of a counted segment is prd.radiance (cell `depth`); on a catcher the occlusion
  test decides prd.alpha instead (the slot's alpha, target 0xffffffff), whether or not the segment counts (:693 comes before
  the BSDF sample).  If the two outcomes agree bit for bit the value is stored and there is no shadow record; otherwise there is
  exactly one shadow record -- origin P, direction wi, the target, val_vis / val_occ the two outcomes -- and the value is
  not stored.  A hit whose BSDF sample has pdf <= 0 (prd DONE) writes no cell.

  Next ray.  From prd.origin along prd.direction with pdf prd.bsdfPdf -- on a pass-through the hit point, the unchanged
  direction and the unchanged pdf -- exactly where the reference traces again and the library does not skip the segment:
  the new depth < max_depth, or the scene holds a catcher.

  Throughput, rayEta, generator.  prd.pathThroughput, prd.rayEta and prd.rand -- compared only for hits that send a next
  ray: nothing reads them otherwise and the kernel leaves them stale (the only exemption; every such hit is DONE or at the
  last depth or was ended by the roulette, which expected() asserts).

  Guides (write_guides).  prd.normal / prd.albedo of a shaded primary hit (:509-512, :653-654).

Everything not named keeps the fill pattern of fovpt_debug_shade."""
import numpy as np

DONE, SECONDARY, ALPHA_ONE, ALPHA_SET = 1, 2, 4, 8
NO_HIT = 0xffffffff
MISS, PASS_THROUGH, SHADED, SHADED_CATCHER = 0, 1, 2, 3


def reference_inputs(h):
    """The hits as the reference holds them: until the first shaded hit pathThroughput is (1, 1, 1) and rayEta 1 (:447-449),
    whatever the library's slot holds."""
    thr = np.array(h["thr"], np.float32, copy=True)
    primary = (h["rng"][:, 2] & SECONDARY) == 0
    thr[primary] = 1.0
    return thr


def oracle_pair(oracle, scene, probe, max_depth, options, h):
    thr = reference_inputs(h)
    return tuple(oracle.shade_hit(scene, probe, max_depth, options, h["origin"], h["dir"], h["prim"], h["tuv"], h["rng"], thr, occ) for occ in (0, 1))


def _bits_equal(a, b):
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) == np.ascontiguousarray(b, np.float32).view(np.uint32)).all(axis=-1)


def expected(h, vis, occ, max_depth, any_catcher, guides):
    """-> dict of per-hit arrays: state (flags | depth << 8), cell (index or -1) and cell_value, alpha_set (bool) and
    alpha_value, shadow (bool), shadow_target, shadow_o / shadow_d / shadow_vis / shadow_occ, next (bool), next_o, next_d (xyz +
    pdf), thr (xyz + eta), rng (two words), guide (bool), guide_n, guide_a."""
    n = len(h["prim"])
    flags_in = (h["rng"][:, 2] & 0xff).astype(np.int64)
    depth_in = (h["rng"][:, 2] >> 8).astype(np.int64)
    kind = vis["kind"]
    # the occlusion test decides radiance and alpha, and nothing else
    for k in ("kind", "flags", "depth", "sky_added", "rr_kill"):
        assert np.array_equal(vis[k], occ[k]), k
    for k in ("origin", "direction", "thr", "normal", "albedo", "P", "wi"):
        assert _bits_equal(vis[k], occ[k]).all(), k
    assert np.array_equal(vis["rng"], occ["rng"])
    shaded = (kind == SHADED) | (kind == SHADED_CATCHER)
    discarded = shaded & (depth_in >= max_depth)                      # the segment the reference traces and throws away
    prd_done = (vis["flags"] & DONE) != 0
    ends = prd_done | (vis["depth"] >= max_depth)                     # :515 (vis depth: the pass-through's is depth - 1)
    sky = (kind == MISS) & (vis["sky_added"] != 0) & (depth_in < max_depth)
    counted = (shaded & ~ends) | sky
    flags = flags_in.copy()
    flags |= np.where(prd_done | discarded, DONE, 0)
    flags |= np.where(shaded, vis["flags"] & SECONDARY, 0)
    flags |= np.where(kind == SHADED, ALPHA_ONE, 0)
    flags |= np.where((kind == SHADED_CATCHER) & ~discarded, ALPHA_SET, 0)
    depth = depth_in + counted
    e = dict(state=(flags | (depth << 8)).astype(np.uint32), kind=kind, counted=counted)
    # value: radiance cell or the slot's alpha; stored, or deferred to a shadow record
    catcher = (kind == SHADED_CATCHER) & ~discarded
    same_rad, same_alpha = _bits_equal(vis["radiance"], occ["radiance"]), _bits_equal(vis["alpha"], occ["alpha"])
    e["shadow"] = (catcher & ~same_alpha) | ((kind == SHADED) & counted & ~same_rad)
    assert same_rad[catcher].all()                                    # (a catcher's radiance is its emission, :696-698)
    e["cell"] = np.where(((kind == SHADED) & counted & same_rad) | (catcher & counted) | sky, depth_in, -1)
    e["cell_value"] = occ["radiance"]
    e["alpha_set"] = catcher & same_alpha
    e["alpha_value"] = occ["alpha"]
    e["shadow_target"] = np.where(catcher, NO_HIT, depth_in).astype(np.uint32)
    e["shadow_o"], e["shadow_d"] = vis["P"], vis["wi"]
    e["shadow_vis"] = np.where(catcher[:, None], vis["alpha"], vis["radiance"])
    e["shadow_occ"] = np.where(catcher[:, None], occ["alpha"], occ["radiance"])
    # next ray
    passes = kind == PASS_THROUGH
    goes_on = (shaded & ~ends & (vis["rr_kill"] == 0)) | passes
    e["next"] = goes_on & (passes | (depth < max_depth) | bool(any_catcher))
    e["next_o"] = np.where(passes[:, None], vis["P"], vis["origin"])
    d = np.where(passes[:, None], h["dir"][:, :3], vis["direction"])
    pdf = np.where(passes, h["dir"][:, 3], vis["bsdfPdf"])
    e["next_d"] = np.concatenate([d, pdf[:, None]], axis=1).astype(np.float32)
    e["thr"] = np.concatenate([vis["thr"], vis["eta"][:, None]], axis=1).astype(np.float32)
    e["rng"] = vis["rng"]
    # the one exemption: a hit that sends no next ray is at the end of its path
    quiet = ~e["next"]
    assert (((flags & DONE) != 0) | (depth >= max_depth) | (vis["rr_kill"] != 0))[quiet].all()
    e["guide"] = bool(guides) & shaded & ~discarded & (depth_in == 0) & ((flags_in & SECONDARY) == 0)
    e["guide_n"], e["guide_a"] = vis["normal"], vis["albedo"]
    assert len(e["state"]) == n
    return e
