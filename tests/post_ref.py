"""fovpt_post restated in numpy float32: the definition the GPU chain (csrc/api_post.hip, the fused kernel of
csrc/post_fused.hip) is checked against.  It is the composition of the stage restatements, nothing else:

    DENOISE      denoise_ref.denoise over the frame's guides
    RECONSTRUCT  reconstruct_ref.reconstruct of the denoised colour, or of the input frame
    TEMPORAL     temporal_motion_ref.step (without MOTION: with no motion record, which is temporal_ref.step) of the previous
                 enabled stage's colour, or of the input frame

so a pixel the reconstruction leaves unchanged reaches the temporal step with its input alpha, and the step outputs it bit for
bit where n == 1."""
import numpy as np

import denoise_ref as dn
import reconstruct_ref as rr
import temporal_motion_ref as tm
import temporal_ref as tr

DENOISE, RECONSTRUCT, TEMPORAL, MOTION = 1, 2, 4, 8          # FOVPT_POST_*
DEFAULT_STAGES = RECONSTRUCT | TEMPORAL | MOTION
VALID_STAGES = tuple(s for s in range(1, 16) if not (s & MOTION and not s & TEMPORAL))


def post(stages, frame, prev=None, cfg=None, motion=None):
    """One fovpt_post call -> dict(color, history, motion, denoised), each (h, w, 4) float32 or None where no enabled stage
    makes it.

    frame: dict of the rendered frame --
        inp                     the chain's colour input (h, w, 4) (unused with DENOISE)
        color, normal, albedo   the frame's guides (DENOISE; albedo also for RECONSTRUCT with remodulate = 1)
        gb, uv                  its G-buffer (prim, position, normal, albedo) and the hit records' (u, v)
        fill, pas, ax, ay       reconstruct_ref.writers() of its passes; uniform: rendered FOV_OFF
        cam                     its camera dict(eye, U, V, W)
    prev: None, or temporal_ref.step's dict(gb, cam, history) of the previous temporal step
    cfg: dict(denoise=, reconstruct=, temporal=) of overrides of the stages' defaults
    motion: None, or temporal_motion_ref.substitute's dict (used with MOTION only)"""
    if stages not in VALID_STAGES:
        raise ValueError("stages %r" % (stages,))
    cfg = cfg or {}
    out = dict(color=None, history=None, motion=None, denoised=None)
    cur = None if stages & DENOISE else np.ascontiguousarray(frame["inp"], np.float32)
    if stages & DENOISE:
        d = dict(dn.DEFAULTS, **(cfg.get("denoise") or {}))
        n = dn.iteration_map(frame["fill"], frame["pas"], d, frame["uniform"])
        cur, _ = dn.denoise(frame["color"], frame["normal"], frame["albedo"], frame["fill"], n, d)
        out["denoised"] = cur
    if stages & RECONSTRUCT:
        cur = rr.reconstruct(cur, frame["albedo"], frame["gb"], frame["fill"], frame["ax"], frame["ay"], cfg.get("reconstruct"))
    if stages & TEMPORAL:
        t = cfg.get("temporal")
        cap = tr.caps(frame["fill"], frame["uniform"], t)
        cur, out["history"], mo = tm.step(cur, frame["gb"], frame["uv"], cap, frame["cam"], prev, t, motion if stages & MOTION else None)
        if stages & MOTION:
            out["motion"] = mo
    out["color"] = cur
    return out
