// fovpt_stream.h -- the one place that says which device memory of a frame is a STREAM: per-ray and per-slot state that one
// kernel writes once and a later kernel reads once, on whichever XCD its wave lands (L2 is per XCD), so that keeping it in
// L1 or L2 serves nobody and only turns the caches over under the scene (nodes, triangles, textures), which IS re-read.
// Shared by the wavefront kernels (wavefront.hip) and the traversal (traverse.hip).  Five classes, each a numeric -D knob with
// its measured default (EXPERIMENTS.md, "After round 4: streams past the caches"):
//
//   FOVPT_STREAM_RAYQ      RayQueue.o / .d
//   FOVPT_STREAM_HIT       PathState.hit
//   FOVPT_STREAM_STATE     PathState.rng, .thr
//   FOVPT_STREAM_SHADOWQ   ShadowQueue.o / .d / .val_vis / .val_occ
//   FOVPT_STREAM_CELLS     PathState.rad, .alpha, .backplate, .guide_n / .guide_a
//
//   0  plain loads and stores
//   1  `nt` loads (served by L2, past L1) and `nt` stores
//   2  `nt` loads, and stores that write through and DROP the line from the XCD's L2 (`sc1`)
//   3  plain loads, `sc1` stores
//   4  plain loads, `nt` stores
//
// Everything else -- nodes, triangles, meshes, tri_tc, textures, probe and guide tables, the Counters, the caller's accum and
// frame -- stays a plain access and is not written through these functions.  A flavour changes where a line lives, never a
// value: kernels hand these streams to each other across kernel boundaries only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef FOVPT_STREAM_RAYQ
#define FOVPT_STREAM_RAYQ 0
#endif
#ifndef FOVPT_STREAM_HIT
#define FOVPT_STREAM_HIT 0
#endif
#ifndef FOVPT_STREAM_STATE
#define FOVPT_STREAM_STATE 0
#endif
#ifndef FOVPT_STREAM_SHADOWQ
#define FOVPT_STREAM_SHADOWQ 0
#endif
#ifndef FOVPT_STREAM_CELLS
#define FOVPT_STREAM_CELLS 4      // nt stores, plain loads: the one class and flavour that measured (C3 frame 0.6555 -> 0.6403 ms);
#endif                            // every other class's best flavour is within noise of plain or slower, and stays plain

// what a class's knob K means for its loads (0 plain, 1 nt) and for its stores (0 plain, 1 nt, 2 sc1)
#define FOVPT_STREAM_LD(K) ((K) == 1 || (K) == 2 ? 1 : 0)
#define FOVPT_STREAM_ST(K) ((K) == 1 || (K) == 4 ? 1 : (K) == 2 || (K) == 3 ? 2 : 0)

namespace {

typedef float StreamF4 __attribute__((ext_vector_type(4)));
typedef uint32_t StreamU4 __attribute__((ext_vector_type(4)));

template <int K>
__device__ inline float4 ld_stream(const float4* p)
{
    static_assert(K >= 0 && K <= 4, "stream knob");
    constexpr int F = FOVPT_STREAM_LD(K);
    if (F == 0) return *p;
    const StreamF4 v = __builtin_nontemporal_load((const StreamF4*)p);
    return make_float4(v.x, v.y, v.z, v.w);
}
template <int K>
__device__ inline uint4 ld_stream(const uint4* p)
{
    static_assert(K >= 0 && K <= 4, "stream knob");
    constexpr int F = FOVPT_STREAM_LD(K);
    if (F == 0) return *p;
    const StreamU4 v = __builtin_nontemporal_load((const StreamU4*)p);
    return make_uint4(v.x, v.y, v.z, v.w);
}
// one 4-byte member of a record
template <int K>
__device__ inline float ld_stream(const float* p) { return FOVPT_STREAM_LD(K) == 0 ? *p : __builtin_nontemporal_load(p); }
template <int K>
__device__ inline uint32_t ld_stream(const uint32_t* p) { return FOVPT_STREAM_LD(K) == 0 ? *p : __builtin_nontemporal_load(p); }

// The 16-byte write-through store has no builtin on a plain pointer: one vector store instruction in an asm statement.  The
// compiler does not count it in its waits (a wait of its own then only waits longer) and does not know when the instruction
// has read its data registers: the s_nop keeps the next instruction off them.
__device__ inline void st_stream_drop(void* p, StreamF4 v)
{
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
}
template <int K>
__device__ inline void st_stream(float4* p, const float4& x)
{
    static_assert(K >= 0 && K <= 4, "stream knob");
    constexpr int F = FOVPT_STREAM_ST(K);
    if (F == 0) { *p = x; return; }
    StreamF4 v;
    v.x = x.x; v.y = x.y; v.z = x.z; v.w = x.w;
    if (F == 1) __builtin_nontemporal_store(v, (StreamF4*)p);
    else st_stream_drop(p, v);
}
template <int K>
__device__ inline void st_stream(uint4* p, const uint4& x)
{
    static_assert(K >= 0 && K <= 4, "stream knob");
    constexpr int F = FOVPT_STREAM_ST(K);
    if (F == 0) { *p = x; return; }
    if (F == 1) {
        StreamU4 v;
        v.x = x.x; v.y = x.y; v.z = x.z; v.w = x.w;
        __builtin_nontemporal_store(v, (StreamU4*)p);
    } else {
        StreamF4 v;
        v.x = __uint_as_float(x.x); v.y = __uint_as_float(x.y); v.z = __uint_as_float(x.z); v.w = __uint_as_float(x.w);
        st_stream_drop(p, v);
    }
}
// one 4-byte member of a record (a relaxed agent-scope atomic store IS the 4-byte write-through vector store)
template <int K>
__device__ inline void st_stream(uint32_t* p, uint32_t x)
{
    static_assert(K >= 0 && K <= 4, "stream knob");
    constexpr int F = FOVPT_STREAM_ST(K);
    if (F == 0) *p = x;
    else if (F == 1) __builtin_nontemporal_store(x, p);
    else __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace
