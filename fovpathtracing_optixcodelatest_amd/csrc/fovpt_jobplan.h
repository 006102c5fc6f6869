// fovpt_jobplan.h -- what the frame engine (run_passes / run_job, fovpt_api.hip) DECIDES about a job before it allocates or
// launches anything: which state set and lane, one chain or two and their halves, how many iterations and shadow-queue buffers,
// which occlusion launch moves to the other lane, the pass table of a job, how an over-budget launch is cut into rows.  Plain
// integer arithmetic on values, with the engine's constants, in one place for the library and for a CPU program
// (tests/cpp/job_plan_test.cpp), which tests/test_job_plan_cpu.py holds to a restatement case by case.  No HIP, no memory, no
// allocation: fovpt_device.h and fovpt_ctx.h include it, and g++ compiles it alone.
#pragma once

#include <stdint.h>

#define FOVPT_BLOCK 256
#define FOVPT_MAX_PASSES 3
#define FOVPT_MAX_ITERS 63         // wavefront iterations per frame (max_depth + catcher pass-throughs)
#define FOVPT_SHARDS 8            // queue shards: one append counter per blockIdx % 8 (~ per XCD)
// Shadow-queue buffers per state set: bounce it writes buffer it % FOVPT_NSQ, so with max_depth <= FOVPT_NSQ the
// main chain never has to wait for an occlusion launch inside a job.
#define FOVPT_NSQ 4
#ifndef FOVPT_LANES_DEFAULT
#define FOVPT_LANES_DEFAULT 2
#endif
#define FOVPT_MAX_LANES 4
#ifndef FOVPT_SETS_SLOT_LIMIT
#define FOVPT_SETS_SLOT_LIMIT (16ull << 20)    // (~330 B of state and queues per slot and set)
#endif

// A queue shard receives the appends of the blocks whose index is congruent to it modulo FOVPT_SHARDS.  The
// producing kernels walk their index space in 256-wide block iterations m = 0, 1, 2, ... with a grid that is
// a multiple of FOVPT_SHARDS, so shard s gets the iterations m = s (mod 8): at most ceil(M / 8) + 1 of them,
// each appending at most 256 entries.  Nothing can overflow a shard of slots / 8 + 512 entries.
inline uint32_t shard_capacity(uint64_t slots) { return (uint32_t)(slots / FOVPT_SHARDS + 512); }

// A launch grid, in blocks: a multiple of FOVPT_SHARDS (shard_capacity() and the work fetch of k_traverse rely on equal shard groups)
inline int shard_grid(int blocks) { return (blocks + FOVPT_SHARDS - 1) / FOVPT_SHARDS * FOVPT_SHARDS; }

// The two chains of a job that plan_job splits (chains_per_frame = 2): chain k takes the sample slots [slot_begin, slot_end) -- the
// first chain a whole number of 256-slot block iterations, the second the rest -- through the queue shards of sel = k + 1.  One
// function for plan_job and for the generate hook of api_debug.hip, so that a test runs the chains a job would issue.
struct ChainSplit { uint32_t sel, slot_begin, slot_end; };
inline ChainSplit chain_split(uint64_t slots, int k)
{
    const uint32_t half = (uint32_t)(slots / 2 / FOVPT_BLOCK * FOVPT_BLOCK);
    ChainSplit s;
    s.sel = k == 0 ? 1u : 2u;
    s.slot_begin = k == 0 ? 0u : half;
    s.slot_end = k == 0 ? half : (uint32_t)slots;
    return s;
}

// ---- plan_job: everything run_job decides between frame_dev and the first launch --------------------------------------------------
// The context's knobs, fixed at creation (FOVPT_LANES, FOVPT_SETS, FOVPT_CHAINS, FOVPT_SPREAD_OCCLUSION) ...
struct PlanKnobs {
    int lanes = FOVPT_LANES_DEFAULT;       // (main, shadow) stream pairs the context made
    unsigned nsets = 4;                    // sets in rotation for ordinary jobs = 2 * lanes (FOVPT_SETS: 2 .. 2 * FOVPT_MAX_LANES)
    int chains_default = 1;                // what fovpt_config.chains_per_frame = 0 means (FOVPT_CHAINS)
    int spread_occlusion = 1;              // sharded frames: one occlusion launch of a first-lane job runs on the second lane's shadow stream (FOVPT_SPREAD_OCCLUSION: 0 off, 1 the last, 2 the second)
};
// ... the rotation so far ...
struct PlanRotation {
    unsigned jobs = 0;                     // jobs issued so far; job j runs on lane j % lanes
    unsigned last_set = 0;                 // the set the most recent job used
};
// ... and the job: the configuration words the plan reads, whether the scene holds a shadow catcher, its sample slots, and
// whether it is a chunk of an over-budget launch
struct PlanJob {
    int frames_in_flight, chains_per_frame, max_depth, world;
    uint32_t any_catcher;
    uint64_t slots;
    int chunked;
};

// One chain: the sample slots [slot_begin, slot_end) through the queue shards of `sel` (0: all eight; 1 / 2: one half), on the
// stream pair of `lane`, with 1 / div of the usual grids.
struct ChainPlan { uint32_t sel, slot_begin, slot_end; unsigned lane; int div; };

struct JobPlan {
    unsigned nrot, set_index;              // the job takes set set_index of a rotation through nrot sets
    unsigned lanes, lane;                  // lanes in use (frames_in_flight), and the one a single chain runs on
    bool two_chains;
    int nchains;                           // 1, or 2 with two_chains
    ChainPlan chain[2];
    int iters, nsq;                        // wavefront iterations, and the shadow-queue buffers they go through
    int spread_it;                         // the iteration whose occlusion launch runs on lane 1's shadow stream; -1: none
};

inline JobPlan plan_job(const PlanKnobs& k, const PlanRotation& r, const PlanJob& j)
{
    JobPlan P;
    // the chunk jobs of an oversized launch all run on lane 0 (their memsets / snapshot copies are ordered on shadow_stream,
    // as before round 3) and, like every job of more than FOVPT_SETS_SLOT_LIMIT sample slots (~330 B of state each), rotate
    // through no more sets than before round 4
    const unsigned few = k.lanes < 2 ? 2u : (unsigned)k.lanes;
    P.nrot = (j.chunked || (unsigned long long)j.slots > FOVPT_SETS_SLOT_LIMIT || k.nsets < few) ? few : k.nsets;
    P.set_index = r.jobs == 0 ? 0u : (r.last_set + 1u) % P.nrot;
    const int fif = j.frames_in_flight > 0 ? j.frames_in_flight : k.lanes;
    P.lanes = (unsigned)(fif < k.lanes ? fif : k.lanes);
    // chains_per_frame = 2: the job is TWO chains -- the halves of its sample slots, each with four of the eight queue shards, on
    // the two lanes -- and one resolve behind both.  (Not for chunk jobs, nor for jobs too small to split.)
    const int chains = j.chains_per_frame > 0 ? j.chains_per_frame : k.chains_default;
    P.two_chains = chains == 2 && k.lanes >= 2 && !j.chunked && j.slots >= 16384;
    P.lane = P.two_chains ? 0u : (P.lanes > 1u && !j.chunked) ? r.jobs % P.lanes : 0u;
    P.nchains = P.two_chains ? 2 : 1;
    for (int n = 0; n < 2; n++) {
        const ChainSplit s = chain_split(j.slots, n);
        P.chain[n] = ChainPlan{s.sel, s.slot_begin, s.slot_end, (unsigned)n, 2};
    }
    if (!P.two_chains) P.chain[0] = ChainPlan{0u, 0u, (uint32_t)j.slots, P.lane, 1};
    // iterations: depth 0 .. max_depth-1, plus the reference's discarded segment and shadow-catcher
    // pass-throughs (which do not advance depth) when the scene holds a catcher
    P.iters = j.max_depth + (j.any_catcher ? 1 + 24 : 0);
    if (P.iters > FOVPT_MAX_ITERS) P.iters = FOVPT_MAX_ITERS;
    P.nsq = P.iters < FOVPT_NSQ ? P.iters : FOVPT_NSQ;        // (only that many shadow queue buffers are allocated)
    // Sharded frames (world > 1): the completion stream -- the first lane's shadow stream -- carries every job's resolve (whose
    // writer search and clearing cover the whole frame on every rank) on top of that lane's occlusion launches and is then as
    // long as the main chains (kernel trace, round 4).  One occlusion launch of a first-lane job moves to the second lane's
    // shadow stream: occlusion launches depend on their shading launch only, and the resolve waits for all of them.
    const bool spread = k.spread_occlusion && j.world > 1 && P.lanes > 1u && P.lane == 0u && !P.two_chains && !j.chunked && j.max_depth >= 2;
    // Which one: a launch is queued when the job is issued and holds the stream's later entries back until its own shading launch
    // has run.  The job's last occlusion launch is the smallest and the resolve waits for it anyway -- but behind it the other
    // lane's next job would find its occlusion launches held back for a whole chain, and with more bounces than shadow queue
    // buffers (iters > FOVPT_NSQ) that job's main chain waits for them (measured: C5, depth 8, 1/8 shard 0.76 -> 1.0 ms).  So:
    // the last launch when no main chain can depend on an occlusion launch, else the second (held back for one bounce only).
    // (FOVPT_SPREAD_OCCLUSION = 2 asks for the second always: A/B.)
    P.spread_it = !spread ? -1 : (k.spread_occlusion == 2 || P.iters > P.nsq) ? 1 : P.iters - 1;
    return P;
}

// ---- the pass table of a job -----------------------------------------------------------------------------------------------------
// Every pass of `in` whole (row1 = 0: its rows 0 .. gh) or its launch rows [row0, row1), as the passes first_pass, first_pass + 1,
// ... of the caller's frame, into `out` (which may be `in`); *slots: the sample slots of the job.  Pass: anything with gw, gh, spp,
// row0, row1 and frame_pass (PassDev; a test's own).  False: a pass without samples (the reference's do{}while(--i) needs one).
template <class Pass> inline bool pass_table(const Pass* in, int npass, uint32_t first_pass, uint32_t row0, uint32_t row1, Pass* out, uint64_t* slots)
{
    *slots = 0;
    for (int p = 0; p < npass; p++) {
        if (in[p].spp == 0) return false;
        Pass& P = out[p];
        P = in[p];
        P.row0 = row1 ? row0 : 0u; P.row1 = row1 ? row1 : P.gh;
        P.frame_pass = first_pass + (uint32_t)p;
        *slots += (uint64_t)P.gw * (P.row1 - P.row0) * P.spp;
    }
    return true;
}

// ---- an over-budget launch, cut into chunks of launch rows -----------------------------------------------------------------------
// The rows per chunk job of a pass of gw launches per row, spp samples each, under a budget of sample slots per job (per_row =
// gw * spp; a pass without launches or samples has no chunks, and the caller skips it).  rows = 0 with per_row > 0: one launch
// row alone needs more than the budget.
struct ChunkRows { uint32_t rows; uint64_t per_row; };
inline ChunkRows chunk_rows(uint64_t budget, uint32_t gw, uint32_t spp)
{
    const uint64_t per_row = (uint64_t)gw * spp;
    return ChunkRows{per_row == 0 || per_row > budget ? 0u : (uint32_t)(budget / per_row), per_row};
}
