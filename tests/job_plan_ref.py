"""What the frame engine decides about a job, restated in numpy from the text of run_job and run_passes (csrc/fovpt_api.hip) as
they stood before the decisions moved into csrc/fovpt_jobplan.h: that text is the authority, not the header.  Every function
takes arrays (or scalars) of equal shape and works on all cases at once; tests/test_job_plan_cpu.py compares the header's answers
(through tests/cpp/job_plan_test.cpp) with these field by field."""
import numpy as np

BLOCK, SHARDS, MAX_ITERS, MAX_PASSES, NSQ, MAX_LANES, LANES_DEFAULT = 256, 8, 63, 3, 4, 4, 2
SETS_SLOT_LIMIT = 16 << 20
TWO_CHAIN_SLOTS = 16384             # a job of fewer sample slots is too small to split
ROW_TEXT = "one launch row needs %d sample slots (budget %d)"
SPP_TEXT = "samples_per_launch must be >= 1"

FIELDS = ("nrot", "set_index", "lanes", "lane", "two_chains", "nchains",
          "sel0", "slot_begin0", "slot_end0", "lane0", "div0", "sel1", "slot_begin1", "slot_end1", "lane1", "div1",
          "iters", "nsq", "spread_it")


def shard_capacity(slots):
    return slots // SHARDS + 512


def plan(slots, lanes, nsets, frames_in_flight, chains_per_frame, chains_default, world, spread_occlusion, max_depth, any_catcher,
         chunked, jobs, last_set):
    """run_job between frame_dev and the first launch: a dict of int64 arrays, one per name of FIELDS."""
    a = [np.asarray(x, np.int64) for x in (slots, lanes, nsets, frames_in_flight, chains_per_frame, chains_default, world,
                                           spread_occlusion, max_depth, any_catcher, chunked, jobs, last_set)]
    slots, lanes, nsets, fif, cpf, cdef, world, spread, depth, catcher, chunked, jobs, last_set = np.broadcast_arrays(*a)
    chunked, catcher = chunked != 0, catcher != 0
    # the state set: chunk jobs, very large jobs and contexts with fewer sets than lanes rotate through one set per lane (two at least)
    few = np.where(lanes < 2, 2, lanes)
    nrot = np.where(chunked | (slots > SETS_SLOT_LIMIT) | (nsets < few), few, nsets)
    set_index = np.where(jobs == 0, 0, (last_set + 1) % nrot)
    # the lanes in use, and whether the job is two chains
    use = np.minimum(np.where(fif > 0, fif, lanes), lanes)
    chains = np.where(cpf > 0, cpf, cdef)
    two = (chains == 2) & (lanes >= 2) & ~chunked & (slots >= TWO_CHAIN_SLOTS)
    lane = np.where(two, 0, np.where((use > 1) & ~chunked, jobs % use, 0))
    # iterations and shadow-queue buffers
    iters = np.minimum(depth + np.where(catcher, 1 + 24, 0), MAX_ITERS)
    nsq = np.minimum(iters, NSQ)
    # the occlusion launch that moves to the second lane's shadow stream: -2 stands for "the job's last one", resolved below
    moves = (spread != 0) & (world > 1) & (use > 1) & (lane == 0) & ~two & ~chunked & (depth >= 2)
    spread_it = np.where(moves, np.where(spread == 2, 1, -2), -1)
    spread_it = np.where(spread_it == -2, np.where(iters <= nsq, iters - 1, 1), spread_it)
    # the chains: one over everything on the job's lane with the whole grids, or the halves on lanes 0 and 1 with half the grids
    half = slots // 2 // BLOCK * BLOCK
    zero = np.zeros_like(slots)
    out = dict(nrot=nrot, set_index=set_index, lanes=use, lane=lane, two_chains=two.astype(np.int64), nchains=np.where(two, 2, 1),
               sel0=np.where(two, 1, 0), slot_begin0=zero, slot_end0=np.where(two, half, slots), lane0=np.where(two, 0, lane),
               div0=np.where(two, 2, 1), sel1=np.where(two, 2, 0), slot_begin1=np.where(two, half, 0), slot_end1=np.where(two, slots, 0),
               lane1=np.where(two, 1, 0), div1=np.where(two, 2, 0), iters=iters, nsq=nsq, spread_it=spread_it)
    assert tuple(out) == FIELDS
    return out


class PlanError(Exception):
    """A launch the engine refuses, with its text."""


def whole_frame(passes):
    """run_passes' table of an unchunked frame from (gw, gh, spp) per pass: rows of (gw, gh, spp, row0, row1, frame_pass), and the
    frame's sample slots."""
    if any(spp == 0 for _, _, spp in passes):
        raise PlanError(SPP_TEXT)
    return [(gw, gh, spp, 0, gh, p) for p, (gw, gh, spp) in enumerate(passes)], sum(gw * gh * spp for gw, gh, spp in passes)


def chunk_jobs(budget, p, gw, gh, spp):
    """The chunk jobs of pass p of an over-budget frame, in issue order: (row0, row1, frame_pass, sample slots) each."""
    per_row = gw * spp
    if per_row == 0 or gh == 0:
        return []
    if per_row > budget:
        raise PlanError(ROW_TEXT % (per_row, budget))
    rows_per = budget // per_row
    return [(y0, min(y0 + rows_per, gh), p, gw * (min(y0 + rows_per, gh) - y0) * spp) for y0 in range(0, gh, rows_per)]


def foveated_passes(w, h, r_inner, r_outer, spp):
    """(gw, gh, spp) of the three launches of a foveated fovpt_render (frame_passes): periphery, middle, fovea."""
    return [(w // 4, h // 4, spp[0]), (r_outer + 2, r_outer + 2, spp[1]), ((r_inner + 1) * 2, (r_inner + 1) * 2, spp[2])]
