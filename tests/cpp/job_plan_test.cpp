// The decisions of the frame engine (csrc/fovpt_jobplan.h) as a stand-alone host program, for tests/test_job_plan_cpu.py: reads
// commands from standard input, one per line, and prints what the header answers.  Built with the address and undefined-behaviour
// sanitizers; no HIP, nothing preloaded.
//
//   consts                      -> BLOCK SHARDS MAX_ITERS MAX_PASSES NSQ MAX_LANES LANES_DEFAULT SETS_SLOT_LIMIT
//   cap SLOTS                   -> shard_capacity
//   grid BLOCKS                 -> shard_grid
//   plans N v.. (12 lists)      -> one line per plan of the PRODUCT of the lists, the last list varying fastest.  The lists, each
//                                  as its length and its values: slots, lanes, nsets, frames_in_flight, chains_per_frame,
//                                  chains_default, world, spread_occlusion, max_depth, any_catcher, chunked, and (jobs, last_set)
//                                  as pairs.  A line: nrot set_index lanes lane two_chains nchains, then per chain sel slot_begin
//                                  slot_end lane div (the second chain of a one-chain job as zeros), then iters nsq spread_it
//   chunks BUDGET FIRST GW GH SPP -> "rows R per_row N", then one line "row0 row1 frame_pass slots" per chunk job, cut and built
//                                  as run_passes does it (chunk_rows, pass_table), then "end"
//   passes ROW0 ROW1 FIRST N (GW GH SPP)xN -> "fail" for a pass without samples, else "slots S" and one line per pass
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "fovpt_jobplan.h"

struct Pass { uint32_t gw, gh, spp, row0, row1, frame_pass; };

static std::vector<long long> read_list(std::istream& in)
{
    size_t n = 0;
    in >> n;
    std::vector<long long> v(n);
    for (auto& x : v) in >> x;
    return v;
}

static void print_plan(const JobPlan& P)
{
    printf("%u %u %u %u %d %d", P.nrot, P.set_index, P.lanes, P.lane, P.two_chains ? 1 : 0, P.nchains);
    for (int k = 0; k < 2; k++) {
        const ChainPlan& c = P.chain[k];
        if (k < P.nchains) printf(" %u %u %u %u %d", c.sel, c.slot_begin, c.slot_end, c.lane, c.div);
        else printf(" 0 0 0 0 0");
    }
    printf(" %d %d %d\n", P.iters, P.nsq, P.spread_it);
}

int main()
{
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "consts") {
            printf("%d %d %d %d %d %d %d %llu\n", FOVPT_BLOCK, FOVPT_SHARDS, FOVPT_MAX_ITERS, FOVPT_MAX_PASSES, FOVPT_NSQ, FOVPT_MAX_LANES,
                   FOVPT_LANES_DEFAULT, (unsigned long long)FOVPT_SETS_SLOT_LIMIT);
        } else if (cmd == "cap") {
            unsigned long long slots = 0;
            std::cin >> slots;
            printf("%u\n", shard_capacity(slots));
        } else if (cmd == "grid") {
            int blocks = 0;
            std::cin >> blocks;
            printf("%d\n", shard_grid(blocks));
        } else if (cmd == "plans") {
            std::vector<long long> L[11];
            for (auto& l : L) l = read_list(std::cin);
            size_t npairs = 0;
            std::cin >> npairs;
            std::vector<long long> jl(2 * npairs);
            for (auto& x : jl) std::cin >> x;
            PlanKnobs k;
            PlanRotation r;
            PlanJob j;
            for (long long slots : L[0]) for (long long lanes : L[1]) for (long long nsets : L[2]) for (long long fif : L[3])
            for (long long cpf : L[4]) for (long long cdef : L[5]) for (long long world : L[6]) for (long long spread : L[7])
            for (long long depth : L[8]) for (long long catcher : L[9]) for (long long chunked : L[10]) for (size_t p = 0; p < npairs; p++) {
                k.lanes = (int)lanes; k.nsets = (unsigned)nsets; k.chains_default = (int)cdef; k.spread_occlusion = (int)spread;
                r.jobs = (unsigned)jl[2 * p]; r.last_set = (unsigned)jl[2 * p + 1];
                j.frames_in_flight = (int)fif; j.chains_per_frame = (int)cpf; j.max_depth = (int)depth; j.world = (int)world;
                j.any_catcher = (uint32_t)catcher; j.slots = (uint64_t)slots; j.chunked = (int)chunked;
                print_plan(plan_job(k, r, j));
            }
        } else if (cmd == "chunks") {
            unsigned long long budget = 0;
            uint32_t first = 0;
            Pass P = {};
            std::cin >> budget >> first >> P.gw >> P.gh >> P.spp;
            const ChunkRows cr = chunk_rows(budget, P.gw, P.spp);
            printf("rows %u per_row %llu\n", cr.rows, (unsigned long long)cr.per_row);
            for (uint32_t y0 = 0; cr.rows && y0 < P.gh; y0 += cr.rows) {
                Pass Q;
                uint64_t slots = 0;
                if (!pass_table(&P, 1, first, y0, y0 + cr.rows < P.gh ? y0 + cr.rows : P.gh, &Q, &slots)) { printf("fail\n"); break; }
                printf("%u %u %u %llu\n", Q.row0, Q.row1, Q.frame_pass, (unsigned long long)slots);
            }
            printf("end\n");
        } else if (cmd == "passes") {
            uint32_t row0 = 0, row1 = 0, first = 0;
            int n = 0;
            std::cin >> row0 >> row1 >> first >> n;
            if (n < 0 || n > FOVPT_MAX_PASSES) return 2;
            Pass in[FOVPT_MAX_PASSES] = {}, out[FOVPT_MAX_PASSES] = {};
            for (int p = 0; p < n; p++) std::cin >> in[p].gw >> in[p].gh >> in[p].spp;
            uint64_t slots = 0;
            if (!pass_table(in, n, first, row0, row1, out, &slots)) { printf("fail\n"); continue; }
            printf("slots %llu\n", (unsigned long long)slots);
            for (int p = 0; p < n; p++) printf("%u %u %u %u %u %u\n", out[p].gw, out[p].gh, out[p].spp, out[p].row0, out[p].row1, out[p].frame_pass);
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
