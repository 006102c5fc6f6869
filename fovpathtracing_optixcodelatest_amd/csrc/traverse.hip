// traverse.hip -- k_traverse, the trace and shadow stages of the wavefront pipeline (wavefront.hip): closest-hit rays
// (optixTrace RADIANCE, deviceProgram.cu:196-222) and occlusion rays (optixTrace OCCLUSION, :224-248,284-300) over the
// 4-wide BVH of bvh_build.hip, and its launcher fovpt_launch_traverse.
//
// Quad-cooperative traversal: FOUR adjacent lanes share one ray.  On a wide node lane j tests child j
// (so a node visit is one box test deep instead of four), on a leaf lane j tests triangle j; the four
// results meet through the wave ballot and DPP quad permutes (register to register).  A wave thus
// carries 16 rays, each step is ~3x shorter than with one lane per ray, and divergence is between 16
// rays instead of 64.  A step is one link of a serial chain per wave -- ~1000 cycles, ~60 % of them the wait for the two node
// loads of the wave's slowest quad, the rest the wave's own ~45 instructions (measured with s_memtime stamps,
// profiles/r03_step_cycles.txt) -- so the steps are written instruction by instruction.
#include "fovpt_device.h"
#include <hip/hip_ext.h>
#include <assert.h>
#include "fovpt_pixel.h"            // V3, cross, dot
#include "fovpt_queue.h"            // ShardMap
#include "fovpt_stream.h"           // ld_stream, st_stream: the once-touched state

// waves per SIMD the traversal kernel is compiled for (caps VGPRs at 64); measured best
#ifndef FOVPT_V_WAVES
#define FOVPT_V_WAVES 8
#endif

namespace {

struct RayT {
    float ox, oy, oz, dx, dy, dz;
    float ix, iy, iz;          // safe reciprocal direction for the box test
    float nox, noy, noz;       // -origin * reciprocal
};

__device__ inline float safe_rcp(float d)
{
    // v_rcp_f32 (1 ulp) is enough: the reciprocal only feeds the conservative box test, whose boxes are
    // padded by >= 1e-5 of the coordinate magnitude at build time (bvh_build.hip, k_tri_bounds)
    const float a = fabsf(d) < 1e-20f ? copysignf(1e-20f, d) : d;
    return __builtin_amdgcn_rcpf(a);
}
__device__ inline void ray_setup(RayT& r, const float4& o, const float4& d)
{
    r.ox = o.x; r.oy = o.y; r.oz = o.z; r.dx = d.x; r.dy = d.y; r.dz = d.z;
    r.ix = safe_rcp(d.x); r.iy = safe_rcp(d.y); r.iz = safe_rcp(d.z);
    r.nox = -o.x * r.ix; r.noy = -o.y * r.iy; r.noz = -o.z * r.iz;
}
// conservative slab test (boxes are padded at build time); returns entry distance in tn.
// (Six scalar fmas: the v_pk_fma_f32 form on (lo, hi) pairs was measured 12 % slower.)
__device__ inline bool box_hit(const RayT& r, float lx, float ly, float lz, float hx, float hy, float hz, float tmin, float tmax, float& tn)
{
    const float ax = __builtin_fmaf(lx, r.ix, r.nox), bx = __builtin_fmaf(hx, r.ix, r.nox);
    const float ay = __builtin_fmaf(ly, r.iy, r.noy), by = __builtin_fmaf(hy, r.iy, r.noy);
    const float az = __builtin_fmaf(lz, r.iz, r.noz), bz = __builtin_fmaf(hz, r.iz, r.noz);
    const float t0 = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), tmin));
    // tmax > 0: as signed integers the bit patterns order like the values whenever one is positive,
    // so the clamp is one v_min_i32 (no canonicalisation of the loop-carried tmax)
    const float far = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
    const float t1 = __int_as_float(min(__float_as_int(far), __float_as_int(tmax)));
    tn = t0;
    // Relative slack: per axis the fma, the rounded -o/d and the 1-ulp reciprocal are off by up to ~2.4e-7
    // of t, independently for the near and the far plane; the build-time padding of the boxes does not
    // cover that for small geometry seen from far away
    return t0 <= t1 * 1.000001f;
}

#define TMIN 0.01f     // deviceProgram.cu:41
#define TMAX 1e16f     // deviceProgram.cu:42

#define TRAV_DONE ((int)0x80000000)     // cur: traversal finished (never a valid leaf code: first_tri < 2^28)

// One ray per quad.  Everything that steers control flow (cur, top, the quad-wide best distance) is
// identical in the four lanes; each lane keeps the best hit among the triangles IT tested and the
// four are merged once, at the end, by (t, primitive id) -- the same total order as a sequential scan.
//
// A node step sits on the wave's dependent chain (load -> test -> rank -> stack -> pop -> load), so it is kept short: the hit mask of the quad comes out of the wave
// ballot (one shift), every lane stores its child at a row derived from its rank and the next node is
// simply popped -- descending and backtracking are the same code, no cross-lane selects.
__device__ inline uint32_t quad_rot1(uint32_t v) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x39, 0xf, 0xf, true); }   // [1,2,3,0]
__device__ inline uint32_t quad_rot2(uint32_t v) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xf, 0xf, true); }   // [2,3,0,1]
__device__ inline uint32_t quad_rot3(uint32_t v) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x93, 0xf, 0xf, true); }   // [3,0,1,2]

enum { ROWB = FOVPT_TQUADS * 4,                 // byte distance of two stack rows
       ROWSHIFT = FOVPT_TQUADS == 16 ? 6 : FOVPT_TQUADS == 64 ? 8 : 10 };
static_assert(FOVPT_LEAF_MAX <= 4, "a leaf is tested in one quad step");
static_assert(FOVPT_TQUADS == 16 || FOVPT_TQUADS == 64 || FOVPT_TQUADS == 256, "row stride of the stack is 64, 256 or 1024 bytes");

// The traversal stack lives in LDS and is addressed through pointers that SAY so (address space 3, 32 bits): every access is a
// ds_read / ds_write by construction.  With a generic `char*` that held only as long as the compiler could infer the address
// space; a build in which it cannot (the stack pointer loaded back from memory, as with a run-time-indexed private array next
// to it -- round 2's faulting diagnostic build) would fall back to flat accesses on a 64-bit pointer.
typedef __attribute__((address_space(3))) char LdsChar;
typedef __attribute__((address_space(3))) int LdsInt;

struct QuadLane {                                   // per-lane constants of the quad traversal
    uint32_t j, qshift, from_me, j32, j3;
    int miss_rows;
    __device__ inline void init()
    {
        j = threadIdx.x & 3u;
        qshift = threadIdx.x & 60u;                 // first lane of this quad within its wave
        from_me = 15u & ~((1u << j) - 1u);          // lanes j..3 of the quad
        j32 = 32u * j; j3 = 3u * j;
        miss_rows = (int)(j + 1u) * ROWB;
    }
};
struct QuadTrav {                                   // state of one ray's traversal (identical in the 4 lanes except the best hit)
    int cur;                                        // node >= 0, leaf < 0, TRAV_DONE
    LdsChar* top;                                   // LDS byte address of the first free stack row
    float lim;                                      // closest: prunes boxes beyond the quad-wide best hit
    float bt, bu, bv; uint32_t bpos, bprim;         // best hit among the triangles THIS lane tested
#if FOVPT_V_STEPSTAT
    uint32_t steps;                                 // diagnostics: node steps | leaf steps << 12 | n0 << 20 of this ray
    uint32_t n0;                                    // node steps in which no child was hit (bits 20-25 of steps)
#endif
    // Row 0 holds the end marker, so "pop" needs no emptiness test; all row arithmetic stays in bytes.
    __device__ inline void start(int* stack, const QuadLane& q)
    {
        if (q.j == 0) stack[0] = TRAV_DONE;
        top = (LdsChar*)(LdsInt*)stack + ROWB;
        cur = 0; lim = TMAX;
        bt = INFINITY; bu = 0.f; bv = 0.f; bpos = 0xffffffffu; bprim = 0xffffffffu;
    }
};

#if FOVPT_V_STEPSTAT
__device__ inline void stepstat(unsigned long long* diag)
{
    const unsigned long long ex = __builtin_amdgcn_ballot_w64(true);
    if ((threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(ex)) { atomicAdd(diag + 0, 1ull); atomicAdd(diag + 1, (unsigned long long)(__builtin_popcountll(ex) >> 2)); }
}
#define STEPSTAT(d) stepstat(d)
#else
#define STEPSTAT(d)
#endif

// The root and its children -- the first FOVPT_TOPN nodes of the breadth-first array, 640 bytes -- live in LDS beside a closest-hit
// wave's stack (4352 + 640 bytes: still eight waves per SIMD), and the first two steps of every ray of a round read them from
// there instead of through the CU's address path: all sixteen rays of a round start at the root together and most go on to one of
// its children, so the two steps are peeled in front of the loop (no per-step choice between the two memories).  Round 4,
// closest-hit launches -1.2 %, frames -1 % (atrium 0.676 -> 0.669, street 1.456 -> 1.439).  Occlusion rays
// start one by one (pool refills): for them a peeled step would be a pass of its own, and they keep the global path.
#define FOVPT_TOPN 5
__shared__ float4 s_top[FOVPT_TOPN * 8];

// A node step, once the lane's child record (a, b) is there: box test, rank, push, pop
template <bool ANY_HIT>
__device__ inline void node_finish(const RayT& r, const QuadLane& q, QuadTrav& T, const float4& a, const float4& b)
{
    const int code = __float_as_int(b.z);
    float t;
    const bool h = box_hit(r, a.x, a.y, a.z, a.w, b.x, b.y, TMIN, T.lim, t);
    const uint32_t m4 = (uint32_t)(__builtin_amdgcn_ballot_w64(h) >> q.qshift) & 15u;
    int Hm1;                                    // H - 1 in one instruction (the compiler splits popcount - 1)
    asm("v_bcnt_u32_b32 %0, %1, -1" : "=v"(Hm1) : "v"(m4));
#if FOVPT_V_STEPSTAT
    if (m4 == 0u) T.n0++;
#endif
    // Every lane stores its child: the H hits land on rows top .. top+H-1 (the one to visit next
    // last), the misses on the free rows above them -- no branch, no select on the address.
    int row;                                    // in bytes, relative to top
    if (ANY_HIT) {
        // storage order (distance order was measured slower)
        row = ((__builtin_popcount(m4 & q.from_me) - 1) << ROWSHIFT) + (h ? 0 : q.miss_rows);
    } else {
        // front to back.  The key orders by entry distance (t >= TMIN > 0: the bit pattern is
        // monotonic) with the lane in the two lowest bits, so keys are distinct and below 2^31
        // (the sign of a difference is the comparison); misses sort first.  The visiting order
        // does not change the result, only the amount of pruning.
        uint32_t key;
        asm("v_and_or_b32 %0, %1, -4, %2" : "=v"(key) : "v"(h ? __float_as_uint(t) : 0u), "v"(__float_as_uint(b.w)));      // b.w: the child's tie rank 0..3 (BvhChild::pad)
        const int lt = ((int)(quad_rot1(key) - key) >> 31) + ((int)(quad_rot2(key) - key) >> 31) + ((int)(quad_rot3(key) - key) >> 31);
        row = (lt << ROWSHIFT) + 3 * ROWB;             // 3 - (number of keys below mine)
    }
    *(LdsInt*)(T.top + row) = code;
    T.top += Hm1 * ROWB;                        // H pushed, one popped
    __builtin_amdgcn_wave_barrier();
    T.cur = *(const LdsInt*)T.top;
}

// wide internal node: lane j owns child j and fetches its record -- from s_top (TOP: the node is one of the first FOVPT_TOPN) or
// through a uniform base + 32-bit offset (fovpt_set_scene keeps nodes and triangles below 4 GB)
template <bool ANY_HIT, bool TOP = false>
__device__ inline void node_step(const SceneView& sc, const RayT& r, const QuadLane& q, QuadTrav& T)
{
    const float4* np = (const float4*)((const char*)sc.nodes + (((uint32_t)T.cur << 7) | q.j32));
    float4 a, b;
    if (TOP) {
        typedef __attribute__((address_space(3))) float LdsFloat;
        const LdsFloat* lp = (const LdsFloat*)((const LdsChar*)(LdsFloat*)(float*)s_top + (((uint32_t)T.cur << 7) | q.j32));
        a = make_float4(lp[0], lp[1], lp[2], lp[3]); b = make_float4(lp[4], lp[5], lp[6], lp[7]);
    } else { a = np[0]; b = np[1]; }
    node_finish<ANY_HIT>(r, q, T, a, b);
}

// A leaf step, once the lane's triangle record is there: Moeller-Trumbore, merge, pop.  Lane j owns triangle j (branch-free:
// the four lanes of 16 rays never agree on an early out); a lane beyond the leaf's count repeats triangle 0: the duplicate
// candidate changes nothing.
// Any-hit: returns true when a front-facing triangle was hit (the ray is occluded, nothing is popped).
template <bool ANY_HIT>
__device__ inline bool leaf_finish(const RayT& r, const QuadLane& q, QuadTrav& T, const TriRec& R, uint32_t tri16)
{
    const V3 d = v3(r.dx, r.dy, r.dz);
    const V3 e1 = v3(R.e1x, R.e1y, R.e1z), e2 = v3(R.e2x, R.e2y, R.e2z);
    const V3 p = cross(d, e2);
    const float det = dot(e1, p);
    const float inv = 1.0f / det;
    const V3 s = v3(r.ox, r.oy, r.oz) - v3(R.v0x, R.v0y, R.v0z);
    const float u = dot(s, p) * inv;
    const V3 qq = cross(s, e1);
    const float v = dot(d, qq) * inv;
    const float t = dot(e2, qq) * inv;
    // the contract's tests; "det != 0" and "u <= 1" are implied: with det == 0 u is +-inf or NaN
    // and then u >= 0 or u + v <= 1 fails; v >= 0 and fl(u + v) <= 1 give u <= 1
    const bool ok = (u >= 0.0f) & (v >= 0.0f) & (u + v <= 1.0f) & (t > TMIN) & (t < TMAX);
    if (ANY_HIT) {
        // front face: counter-clockwise seen from the origin
        if ((uint32_t)(__builtin_amdgcn_ballot_w64(ok & (det > 0.0f)) >> q.qshift) & 15u) return true;
    } else {
        const bool better = ok & ((t < T.bt) | ((t == T.bt) & (R.prim < T.bprim)));
        T.bt = better ? t : T.bt; T.bu = better ? u : T.bu; T.bv = better ? v : T.bv;
        T.bpos = better ? tri16 : T.bpos; T.bprim = better ? R.prim : T.bprim;
        // quad-wide best: bt > 0 or +inf, so the bit patterns order like the values
        uint32_t m = __float_as_uint(T.bt);
        m = min(m, quad_rot2(m));
        m = min(m, quad_rot1(m));
        T.lim = fminf(TMAX, __uint_as_float(m) * 1.000001f);
    }
    T.top -= ROWB;
    T.cur = *(const LdsInt*)T.top;
    return false;
}

// A MIXED step (round 4): the pass the wave makes when its vote ends a node phase.  The rays waiting at a leaf test their
// triangles -- and the rays still at a node step theirs in the same pass, behind the SAME wait for memory: nodes and triangles
// live in one allocation, so every live lane fetches 48 bytes from one base register (a node lane's third 16 bytes are not
// used), then the node lanes and the leaf lanes finish their step one after the other.  The instructions are the ones two
// separate passes would issue; what goes is one memory round trip and the idling of the node lanes through a leaf step.
// Any-hit: returns true for a quad whose leaf step found an occluder.
template <bool ANY_HIT>
__device__ inline bool mixed_step(const SceneView& sc, const RayT& r, const QuadLane& q, QuadTrav& T, unsigned long long* diag)
{
    const bool at_node = T.cur >= 0;
    const uint32_t lcode = (uint32_t)~T.cur;
    const uint32_t tri16 = (lcode >> 3) + (q.j <= (lcode & 7u) ? q.j3 : 0u);
    const uint32_t off = at_node ? (((uint32_t)T.cur << 7) | q.j32) : sc.tri_off + (tri16 << 4);
    const float4* p = (const float4*)((const char*)sc.nodes + off);
    const float4 x0 = p[0], x1 = p[1], x2 = p[2];
    if (at_node) {
        STEPSTAT(diag);
        node_finish<ANY_HIT>(r, q, T, x0, x1);
        return false;
    }
    STEPSTAT(diag + 2);
    TriRec R;
    R.v0x = x0.x; R.v0y = x0.y; R.v0z = x0.z; R.e1x = x0.w;
    R.e1y = x1.x; R.e1z = x1.y; R.e2x = x1.z; R.e2y = x1.w;
    R.e2z = x2.x; R.prim = __float_as_uint(x2.y); R.mesh = __float_as_uint(x2.z); R.pad = 0;
    return leaf_finish<ANY_HIT>(r, q, T, R, tri16);
}

// closest: store the hit record of the quad's ray AT THE RAY'S QUEUE POSITION (the shading kernel reads ray and
// hit side by side).  Lowest t (bit patterns of t > 0 order like the
// values), then lowest primitive id; lanes that tie on both hold the same triangle, hence the same
// record: they all store it.
__device__ inline void store_hit(const PathState& ps, uint32_t ph, const QuadTrav& T)
{
    uint32_t mt = __float_as_uint(T.bt);
    mt = min(mt, quad_rot2(mt));
    mt = min(mt, quad_rot1(mt));
    const bool cand = __float_as_uint(T.bt) == mt;
    uint32_t mp = cand ? T.bprim : 0xffffffffu;
    mp = min(mp, quad_rot2(mp));
    mp = min(mp, quad_rot1(mp));
    if (cand && T.bprim == mp) st_stream<FOVPT_STREAM_HIT>(ps.hit + ph, make_float4(T.bt, T.bu, T.bv, __uint_as_float(T.bpos)));
}
// any-hit: the deferred NEE add of SampleLights / SampleShadow (deviceProgram.cu:323-341,367-385).
// Every (slot, depth) cell has exactly one writer, so this is a plain store and the shadow rays of a
// bounce may run at any time before resolve (own stream, see fovpt_api.hip)
__device__ inline void store_shadow(const PathState& ps, const ShadowQueue& sq, uint32_t ph, uint32_t slot, uint32_t target, bool occluded)
{
    const float4 val = occluded ? ld_stream<FOVPT_STREAM_SHADOWQ>(sq.val_occ + ph) : ld_stream<FOVPT_STREAM_SHADOWQ>(sq.val_vis + ph);
    float4* cell = target == 0xffffffffu ? ps.alpha + slot : ps.rad + ((size_t)slot * ps.stride + target);
    st_stream<FOVPT_STREAM_CELLS>(cell, make_float4(val.x, val.y, val.z, 0.f));
}

// na live lanes of the wave, nn of them at a node: does the node phase end here?  (FOVPT_VOTE_C = 64: never -- the phases of rounds 1-3)
#ifndef FOVPT_VOTE_A
#define FOVPT_VOTE_A 2
#endif
#ifndef FOVPT_VOTE_B
#define FOVPT_VOTE_B 1
#endif
#ifndef FOVPT_VOTE_C
#define FOVPT_VOTE_C 1
#endif
__device__ inline bool vote_leaf(uint32_t na, uint32_t nn)
{
    return (na - nn) * (uint32_t)FOVPT_VOTE_A >= nn * (uint32_t)FOVPT_VOTE_B + 4u * (uint32_t)FOVPT_VOTE_C;
}

__device__ inline void traverse_quad(const SceneView& sc, const RayT& r, int* __restrict__ stack /* [e * QUADS_PER_BLOCK] */, const QuadLane& q,
                              QuadTrav& T, unsigned long long* diag)
{
    T.start(stack, q);
    // The wave VOTES when its node phase ends (round 4).  Rounds 1-3 ran node steps until EVERY ray of the wave had reached a leaf (or
    // was through): a ray at a leaf waited for the longest run of node steps among the other fifteen, and only 8.3 (atrium) / 5.8
    // (street) of the 16 rays took part in an average node step.  Now the phase ends as soon as the rays waiting at a leaf
    // outnumber those still stepping (vote_leaf: waiting x A >= stepping x B + C quads): a leaf step then serves the waiting rays,
    // the stepping ones sit it out and go on afterwards.  Leaf steps get emptier (9.3 -> 5.2 rays of 16, and 77 % more of them),
    // node steps fuller (8.3 -> 10.6, 22 % fewer): in node-step units (a leaf step costs 1.4) a wave's passes fall by 7 % on the
    // atrium and by 27 % on the street.  The vote rides on what the loop computes anyway -- the lanes that go on are the loop's
    // own exit mask, one s_bcnt1 and six scalar instructions -- after a first form with a ballot per state and a branch per pass
    // cost 12-15 % per pass and lost on the atrium (EXPERIMENTS.md).  Order of steps never changes a result.
#if FOVPT_V_STEPSTAT
    // (no arrays with a run-time index here: a diagnostic build whose traversal kernel used scratch memory faulted with
    // HSA_STATUS_ERROR_MEMORY_APERTURE_VIOLATION on the closest-hit launch; the product kernels use none)
    uint32_t my_nodes = 0u, my_leaves = 0u;          // this ray's own steps (tools/stepcount.py, raystat.py)
    T.n0 = 0u;
#define RAYSTAT(x) (x)++
#else
#define RAYSTAT(x)
#endif
    // every ray of a round starts at the root, and most go on to one of its children: those two steps out of LDS
    if (sc.num_nodes >= FOVPT_TOPN) {
        STEPSTAT(diag);
        node_step<false, true>(sc, r, q, T);
        RAYSTAT(my_nodes);
        if (T.cur >= 0 && T.cur < FOVPT_TOPN) { STEPSTAT(diag); node_step<false, true>(sc, r, q, T); RAYSTAT(my_nodes); }
    }
    while (T.cur != TRAV_DONE) {                                                                         // (rays that are through leave)
        const uint32_t na = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(true));            // live lanes of the wave
        while (T.cur >= 0) {
            STEPSTAT(diag);
            node_step<false>(sc, r, q, T);
            RAYSTAT(my_nodes);
            const uint32_t nn = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(T.cur >= 0));   // of the lanes that stepped: who goes on
            if (vote_leaf(na, nn)) break;                                                                  // (wave-uniform)
        }
        if (T.cur != TRAV_DONE) {
#if FOVPT_V_STEPSTAT
            if (T.cur >= 0) my_nodes++; else my_leaves++;
#endif
            mixed_step<false>(sc, r, q, T, diag);
        }
    }
#if FOVPT_V_STEPSTAT
    T.steps = min(my_nodes, 4095u) | (min(my_leaves, 255u) << 12) | (min(T.n0, 63u) << 20);
#endif
#undef RAYSTAT
}

// Any-hit traversal over a POOL of shadow rays [first, end) owned by one wave: a quad that has finished
// its ray takes the next one of the pool as soon as FOVPT_REFILL quads of the wave are idle (all of them
// at the end), so the wave does not wait for its longest ray after every 16 -- occlusion rays end after
// very different numbers of steps (SIMD utilisation 36 % with static rounds).  The pool is private to
// the wave: no atomics.  (For closest-hit rays the same scheme was measured 10 % slower: the divergent
// refill -- merge and store the hit, fetch, set up -- costs more than their better lane use returns.)
#ifndef FOVPT_REFILL
#define FOVPT_REFILL 6
#endif
__device__ inline void traverse_shadow_pool(const SceneView& sc, const PathState& ps, const ShadowQueue& sq, const ShardMap& map, uint32_t cap,
                                            uint32_t first, uint32_t end, int* __restrict__ stack, const QuadLane& q, unsigned long long* diag)
{
    QuadTrav T;
    T.start(stack, q);
    T.cur = TRAV_DONE;
    RayT r = {};
    uint32_t ph = 0;                              // physical index of the quad's shadow record
    bool pending = false, occluded = false;
    uint32_t next = first;
    for (;;) {
        const unsigned long long idle = __builtin_amdgcn_ballot_w64(T.cur == TRAV_DONE);
        const uint32_t n_idle = (uint32_t)__builtin_popcountll(idle) >> 2;
        if (n_idle == 16u || (n_idle >= (uint32_t)FOVPT_REFILL && next < end)) {
            if (T.cur == TRAV_DONE) {
                if (pending && q.j == 0) store_shadow(ps, sq, ph, __float_as_uint(ld_stream<FOVPT_STREAM_SHADOWQ>(&sq.o[ph].w)),
                                                          __float_as_uint(ld_stream<FOVPT_STREAM_SHADOWQ>(&sq.d[ph].w)), occluded);
                pending = false;
                // idle quads below mine (all four lanes of an idle quad are set in the mask)
                const uint32_t rank = (__builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u)) - q.j) >> 2;
                const uint32_t idx = next + rank;
                if (idx < end) {
                    ph = map.phys16(idx, next, cap);
                    ray_setup(r, ld_stream<FOVPT_STREAM_SHADOWQ>(sq.o + ph), ld_stream<FOVPT_STREAM_SHADOWQ>(sq.d + ph));
                    T.start(stack, q);
                    pending = true; occluded = false;
                }
            }
            next = min(end, next + n_idle);
            if (n_idle == 16u && __builtin_amdgcn_ballot_w64(T.cur != TRAV_DONE) == 0ull) return;      // pool exhausted, all results stored
        }
        // the same vote as for closest-hit rays (traverse_quad); the live lanes are the quads that hold a ray
        const uint32_t na = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(T.cur != TRAV_DONE));
        while (T.cur >= 0) {
            STEPSTAT(diag);
            node_step<true>(sc, r, q, T);
            const uint32_t nn = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(T.cur >= 0));
            if (vote_leaf(na, nn)) break;
        }
        if (T.cur != TRAV_DONE) {
            if (mixed_step<true>(sc, r, q, T, diag)) { occluded = true; T.cur = TRAV_DONE; }
        }
    }
}

// One traversal launch handles the closest-hit rays of iteration it_closest (MODE 0) or the occlusion rays of
// iteration it_shadow (MODE 1), one ray per QUAD of lanes (16 rays per wave); the other iteration is not read.
// (Dynamic work fetching with a global counter and per-lane replacement was measured and rejected: with
// so few rays per resident lane per launch a returning atomic per wave costs more than the imbalance.)
// (A build of the kernel for each, so that a wave of a closest-hit launch neither fetches the occlusion queue's shard sizes
// before it starts nor carries that loop's registers.)
template <int MODE>
__global__ __launch_bounds__(FOVPT_TBLOCK, FOVPT_V_WAVES) void k_traverse(SceneView sc, PathState ps, RayQueue queue, ShadowQueue sq,
                                                                         uint32_t cap, Counters* __restrict__ cnt, int it_closest, int it_shadow, uint32_t sel)
{
    __shared__ int s_stack[(FOVPT_STACK + 4) * FOVPT_TQUADS];  // + the end marker and three rows of slack above the top
    static_assert(MODE == 0 || MODE == 1, "closest hit or occlusion");
    const int it = MODE == 0 ? it_closest : it_shadow;
    ShardMap map;                                               // of the one queue this launch reads
    map.load(cnt, MODE == 0 ? FOVPT_CNT_Q(it >= 0 ? it : 0) : FOVPT_CNT_SQ(it >= 0 ? it : 0), sel, cap);
    const uint32_t n_cl = (MODE == 0 && it >= 0) ? map.total() : 0u;
    const uint32_t n_sh = (MODE == 1 && it >= 0) ? map.total() : 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (n_cl) atomicAdd(&cnt->stat_radiance, (unsigned long long)n_cl);
        if (n_sh) atomicAdd(&cnt->stat_shadow, (unsigned long long)n_sh);
        if (MODE == 0 && it == 0) atomicAdd(&cnt->stat_paths, (unsigned long long)n_cl);
    }
    QuadLane q;
    q.init();
    int* stack = s_stack + (threadIdx.x >> 2);
    if (MODE == 0 && sc.num_nodes >= FOVPT_TOPN) {
        for (uint32_t k = threadIdx.x; k < FOVPT_TOPN * 8u; k += FOVPT_TBLOCK) s_top[k] = ((const float4*)sc.nodes)[k];
        __syncthreads();
    }
    // occlusion rays: every wave owns one contiguous pool
    if (n_sh) {
        const uint32_t nwaves = gridDim.x * (FOVPT_TBLOCK / 64), wave = blockIdx.x * (FOVPT_TBLOCK / 64) + (threadIdx.x >> 6);
        const uint32_t per = (n_sh + nwaves - 1u) / nwaves, first = min(n_sh, wave * per);
        traverse_shadow_pool(sc, ps, sq, map, cap, first, min(n_sh, first + per), stack, q, cnt->diag[1]);
    }
    // closest-hit rays: static grid-stride over quads, 16 consecutive rays per wave and round
    const uint32_t quads = gridDim.x * FOVPT_TQUADS;
    for (uint32_t i = blockIdx.x * FOVPT_TQUADS + (threadIdx.x >> 2); i < n_cl; i += quads) {
        const uint32_t i0 = __builtin_amdgcn_readfirstlane(i - ((threadIdx.x & 63u) >> 2));      // the wave's 16 rays: i0 .. i0+15
        RayT r;
        QuadTrav T;
        const uint32_t ph = map.phys16(i, i0, cap);
        const float4 o = ld_stream<FOVPT_STREAM_RAYQ>(queue.o + ph), d = ld_stream<FOVPT_STREAM_RAYQ>(queue.d + ph);
        ray_setup(r, o, d);
        traverse_quad(sc, r, stack, q, T, cnt->diag[0]);
        store_hit(ps, ph, T);
#if FOVPT_V_STEPSTAT
        if (q.j == 0) ((uint32_t*)&queue.d[ph])[3] = T.steps;             // tools/raystat.py, raytrace_dump.py
#endif
    }
}

}  // namespace

void fovpt_launch_traverse(hipStream_t st, SceneView sc, PathState ps, RayQueue queue, ShadowQueue sq, uint32_t cap,
                           Counters* cnt, int it_closest, int it_shadow, int grid, hipEvent_t done, uint32_t sel)
{
    // One queue per launch: a call with both iterations set is the caller's mistake and is asserted on, not rejected (no
    // caller ever traced both in one launch, and the build of the kernel that could is gone).
    assert(it_closest < 0 || it_shadow < 0);
    // `done` rides on the kernel's own completion signal (no separate marker packet in the queue)
    // (`grid` counts blocks of 256 threads, as for the other kernels; the traversal block may be larger)
    int blocks = grid * FOVPT_BLOCK / FOVPT_TBLOCK > 0 ? grid * FOVPT_BLOCK / FOVPT_TBLOCK : 1;
    if (it_shadow < 0) {
        // a closest-hit launch reads at most 8 * cap rays (the shards' capacities): no more workgroups than it can have rounds of
        // FOVPT_TQUADS rays (what matters for the small frames of a 1/N shard)
        const unsigned long long rounds = ((sel ? 4ull : 8ull) * cap + FOVPT_TQUADS - 1) / FOVPT_TQUADS;
        if ((unsigned long long)blocks > rounds) blocks = (int)((rounds + FOVPT_SHARDS - 1) / FOVPT_SHARDS * FOVPT_SHARDS);
    }
    auto kernel = it_shadow < 0 ? k_traverse<0> : k_traverse<1>;
    if (done) hipExtLaunchKernelGGL(kernel, dim3(blocks), dim3(FOVPT_TBLOCK), 0, st, nullptr, done, 0, sc, ps, queue, sq, cap, cnt, it_closest, it_shadow, sel);
    else hipLaunchKernelGGL(kernel, dim3(blocks), dim3(FOVPT_TBLOCK), 0, st, sc, ps, queue, sq, cap, cnt, it_closest, it_shadow, sel);
}
