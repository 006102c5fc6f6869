// fovpt_queue.h -- reading the sharded ray queues on the device, shared by the wavefront kernels (wavefront.hip) and the
// traversal (traverse.hip): which shards a launch works in, and the map from a logical queue index to its physical place.
// (Counters and the queues themselves: fovpt_device.h.)
#pragma once

#include "fovpt_device.h"

namespace {

// Shard selection of a launch: 0 = all eight shards; 1 / 2 = the first / second four -- the two CHAINS of a frame that is rendered
// as two independent halves (fovpt_config.chains_per_frame = 2, fovpt_api.hip): each chain's kernels read and append only inside
// their own four shards of the same queue buffers.
__device__ inline uint32_t sel_first(uint32_t sel) { return sel == 2u ? 4u : 0u; }
__device__ inline uint32_t sel_mask(uint32_t sel) { return sel == 0u ? (uint32_t)FOVPT_SHARDS - 1u : 3u; }

// logical index -> physical index of a sharded queue (all in scalar registers, no indexing)
struct ShardMap {
    uint32_t p1, p2, p3, p4, p5, p6, p7, p8;     // exclusive prefix sums of the shard counts (p0 = 0)
    uint32_t first_cap;                          // physical offset of the first shard of the selection (0, or 4 * cap for the second chain)
    __device__ inline void load(const Counters* cnt, int word, uint32_t sel = 0u, uint32_t cap = 0u)
    {
        const uint32_t f = sel_first(sel);
        first_cap = f * cap;
        p1 = cnt->shard[f][word]; p2 = p1 + cnt->shard[f + 1][word]; p3 = p2 + cnt->shard[f + 2][word]; p4 = p3 + cnt->shard[f + 3][word];
        if (sel == 0u) { p5 = p4 + cnt->shard[4][word]; p6 = p5 + cnt->shard[5][word]; p7 = p6 + cnt->shard[6][word]; p8 = p7 + cnt->shard[7][word]; }
        else p5 = p6 = p7 = p8 = p4;             // a chain's four shards: no index reaches the other four
    }
    __device__ inline uint32_t total() const { return p8; }
    __device__ inline uint32_t phys(uint32_t i, uint32_t cap) const
    {
        uint32_t s = 0, base = 0;
        if (i >= p1) { s = 1; base = p1; }
        if (i >= p2) { s = 2; base = p2; }
        if (i >= p3) { s = 3; base = p3; }
        if (i >= p4) { s = 4; base = p4; }
        if (i >= p5) { s = 5; base = p5; }
        if (i >= p6) { s = 6; base = p6; }
        if (i >= p7) { s = 7; base = p7; }
        return first_cap + s * cap + (i - base);
    }
    // the same for lane index i of 16 consecutive indices starting at the wave-uniform i0: the shard is
    // found with scalar instructions unless the 16 straddle a shard boundary
    __device__ inline uint32_t phys16(uint32_t i, uint32_t i0, uint32_t cap) const
    {
        uint32_t s = 0, base = 0, next = p1;
        if (i0 >= p1) { s = 1; base = p1; next = p2; }
        if (i0 >= p2) { s = 2; base = p2; next = p3; }
        if (i0 >= p3) { s = 3; base = p3; next = p4; }
        if (i0 >= p4) { s = 4; base = p4; next = p5; }
        if (i0 >= p5) { s = 5; base = p5; next = p6; }
        if (i0 >= p6) { s = 6; base = p6; next = p7; }
        if (i0 >= p7) { s = 7; base = p7; next = 0xffffffffu; }
        if (i0 + 15u < next) return first_cap + s * cap - base + i;
        return phys(i, cap);
    }
};

}  // namespace
