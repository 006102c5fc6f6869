// wavefront.hip -- the foveated path-tracing launch as a wavefront pipeline on gfx950.
//
// What the reference runs as ONE OptiX raygen thread per launch index with recursive
// optixTrace calls (PT_sv5_/deviceProgram.cu:392-732) is split here into queue-driven stages,
// one sample *slot* = (pass, launch index, sample number) per work item:
//
//   generate      __raygen__renderFrame :394-495   seed, ring test, jitter, camera ray, backplate
//   trace         optixTrace RADIANCE   :196-222   closest hit over the 4-wide BVH, LDS-staged stack: k_traverse<0>, traverse.hip
//   shade         __closesthit__/__miss__radiance :253-282,619-732 + SampleLights :303-344
//                 + Disney BSDF (Disney.cuh) + probe NEE (Probe.cuh); emits the shadow ray and
//                 the continuation ray, ballot-compacted into the next queues
//   shadow        optixTrace OCCLUSION  :224-248,284-300   any front-facing candidate: k_traverse<1>, traverse.hip
//   resolve       :541-616              ordered per-launch sample reduction, pass-ordered
//                                       block fill, exposure, Reinhard, sRGB, rgba8
//
// The three foveation passes of SampleRenderer::render() (SimplePathtracer.cpp:133-213) are
// one job: their slots share the queues, and resolve gives every pixel to its last writer in
// the reference's launch order (P, then M, then F; within a launch ascending y, x).
//
// Arithmetic: fp32 with the reference's operation order, -ffp-contract=off, IEEE divide and
// sqrt, transcendental functions from include/fovpt_detmath.h.  The only fused multiply-adds
// are the explicit ones in the (conservative) box test.
#include "fovpt_device.h"
#include <hip/hip_ext.h>
#include "../../include/fovpt_detmath.h"
#include "fovpt_pixel.h"            // V3, ring_alive, find_last_writer, the tone map (shared with denoise.hip)
#include "fovpt_scene.h"            // load_tri_off, tex2d (shared with reconstruct.hip)
#include "fovpt_queue.h"            // sel_first, sel_mask, ShardMap (shared with traverse.hip)
#include "fovpt_stream.h"           // ld_stream, st_stream: the once-touched state (shared with traverse.hip)
#include "fovpt_shade_fn.h"         // Rng, the probe, the Disney BSDF (shared with shade_debug.hip)

namespace {

// ------------------------------------------------------------------------------------------
// wavefront plumbing
// ------------------------------------------------------------------------------------------
// Ballot compaction into a sharded queue.  Lanes with pred get distinct positions inside shard
// blockIdx % 8: wave ballot + popcount prefix, the four wave totals meet in LDS, and ONE atomic per
// block-iteration reserves the range.  Must be called by all 256 threads of the block (two barriers).
// (sel: the shards of the launch, fovpt_queue.h)
__device__ inline uint32_t block_append(Counters* cnt, int word, uint32_t cap, bool pred, uint32_t* s_scratch /* [6] */, uint32_t sel = 0u)
{
    const unsigned long long mask = __ballot(pred);
    const uint32_t lane = __lane_id();
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t prefix = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) s_scratch[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    const uint32_t c0 = s_scratch[0], c1 = s_scratch[1], c2 = s_scratch[2], c3 = s_scratch[3];
    const uint32_t shard = sel_first(sel) + (blockIdx.x & sel_mask(sel));
    if (threadIdx.x == 0) {
        const uint32_t total = c0 + c1 + c2 + c3;
        s_scratch[4] = total ? atomicAdd(&cnt->shard[shard][word], total) : 0u;
    }
    __syncthreads();
    const uint32_t before = (wave > 0 ? c0 : 0u) + (wave > 1 ? c1 : 0u) + (wave > 2 ? c2 : 0u);
    const uint32_t pos = shard * cap + s_scratch[4] + before + prefix;
    __syncthreads();                 // s_scratch is reused by the next call
    return pos;
}

// Two appends at once (shadow queue and next radiance queue) behind ONE pair of barriers.
__device__ inline void block_append2(Counters* cnt, int word_a, bool pred_a, int word_b, bool pred_b, uint32_t cap,
                                     uint32_t* s_scratch /* [10] */, uint32_t& pos_a, uint32_t& pos_b, uint32_t sel = 0u)
{
    const unsigned long long ma = __ballot(pred_a), mb = __ballot(pred_b);
    const uint32_t lane = __lane_id();
    const uint32_t wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t pa = __popcll(ma & below), pb = __popcll(mb & below);
    if (lane == 0) { s_scratch[wave] = (uint32_t)__popcll(ma); s_scratch[4 + wave] = (uint32_t)__popcll(mb); }
    __syncthreads();
    const uint32_t a0 = s_scratch[0], a1 = s_scratch[1], a2 = s_scratch[2], a3 = s_scratch[3];
    const uint32_t b0 = s_scratch[4], b1 = s_scratch[5], b2 = s_scratch[6], b3 = s_scratch[7];
    const uint32_t shard = sel_first(sel) + (blockIdx.x & sel_mask(sel));
    if (threadIdx.x == 0) {
        const uint32_t ta = a0 + a1 + a2 + a3;
        s_scratch[8] = ta ? atomicAdd(&cnt->shard[shard][word_a], ta) : 0u;
    }
    if (threadIdx.x == 64) {
        const uint32_t tb = b0 + b1 + b2 + b3;
        s_scratch[9] = tb ? atomicAdd(&cnt->shard[shard][word_b], tb) : 0u;
    }
    __syncthreads();
    pos_a = shard * cap + s_scratch[8] + (wave > 0 ? a0 : 0u) + (wave > 1 ? a1 : 0u) + (wave > 2 ? a2 : 0u) + pa;
    pos_b = shard * cap + s_scratch[9] + (wave > 0 ? b0 : 0u) + (wave > 1 ? b1 : 0u) + (wave > 2 ? b2 : 0u) + pb;
    __syncthreads();                 // s_scratch is reused by the next iteration
}

// The same with the SECOND append partitioned inside the block's range by one bit of the entry: class 0 first, then class 1.
// k_shade uses it for the next bounce's rays with the sign of dir.y as the class: the 16 consecutive rays of a traversal round then
// point more nearly the same way and need more nearly the same number of steps.  It is the block-local form of a direction-sorted
// queue -- no extra memory, no extra atomics, ~12 instructions per 256 rays -- and queue order never changes a result (every ray
// writes to its own slot).  Measured: foveated frames -1 % (C3, street), the uniform 1-spp frame +1 %: on for foveated frames only.
__device__ inline void block_append2d(Counters* cnt, int word_a, bool pred_a, int word_b, bool pred_b, bool cls_b, uint32_t cap,
                                      uint32_t* s_scratch /* [14] */, uint32_t& pos_a, uint32_t& pos_b, uint32_t sel = 0u)
{
    const unsigned long long ma = __ballot(pred_a), mb0 = __ballot(pred_b & !cls_b), mb1 = __ballot(pred_b & cls_b);
    const uint32_t lane = __lane_id();
    const uint32_t wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t pa = __popcll(ma & below), pb = __popcll((cls_b ? mb1 : mb0) & below);
    if (lane == 0) { s_scratch[wave] = (uint32_t)__popcll(ma); s_scratch[4 + wave] = (uint32_t)__popcll(mb0); s_scratch[8 + wave] = (uint32_t)__popcll(mb1); }
    __syncthreads();
    const uint32_t a0 = s_scratch[0], a1 = s_scratch[1], a2 = s_scratch[2], a3 = s_scratch[3];
    uint32_t before_b = 0u, tb0 = 0u, tb1 = 0u;
#pragma unroll
    for (uint32_t w = 0; w < 4u; w++) {
        const uint32_t b0 = s_scratch[4 + w], b1 = s_scratch[8 + w];
        if (w < wave) before_b += cls_b ? b1 : b0;
        tb0 += b0; tb1 += b1;
    }
    const uint32_t shard = sel_first(sel) + (blockIdx.x & sel_mask(sel));
    if (threadIdx.x == 0) {
        const uint32_t ta = a0 + a1 + a2 + a3;
        s_scratch[12] = ta ? atomicAdd(&cnt->shard[shard][word_a], ta) : 0u;
    }
    if (threadIdx.x == 64) s_scratch[13] = (tb0 + tb1) ? atomicAdd(&cnt->shard[shard][word_b], tb0 + tb1) : 0u;
    __syncthreads();
    pos_a = shard * cap + s_scratch[12] + (wave > 0 ? a0 : 0u) + (wave > 1 ? a1 : 0u) + (wave > 2 ? a2 : 0u) + pa;
    pos_b = shard * cap + s_scratch[13] + (cls_b ? tb0 : 0u) + before_b + pb;
    __syncthreads();                 // s_scratch is reused by the next iteration
}

// p: index of the pass within this JOB; the rotation uses its index within the caller's FRAME (a chunked frame runs every
// pass as jobs of its own, and the gather plan is made for the frame)
__device__ inline bool launch_owned(const FrameDev& fd, int p, uint32_t lx, uint32_t ly)
{
    if (fd.world <= 1) return true;
    uint32_t tx = lx / (uint32_t)fd.tile_w, ty = ly / (uint32_t)fd.tile_h;
    return (int)((tx + 3u * ty + fd.pass[p].frame_pass) % (uint32_t)fd.world) == fd.rank;
}

// ---- generate ----------------------------------------------------------------------------
// A rank's share of pass P in the tile-sharded frame, as an index space of its own: tile rows x the rank's tiles of a row
// (every world-th tile, launch_owned) x the tile's launch indices x samples.  k_generate<true> walks it instead of all sample
// slots -- 1 / world of the work; the sample slot of a launch index, and so everything downstream, is the same.
struct OwnedSpace {
    uint32_t ty0, tile_rows, per_row, tile_lis, count;      // first tile row, tile rows, the rank's tiles per tile row (at most), launch indices per tile
    __host__ __device__ inline void init(const FrameDev& fd, const PassDev& P)
    {
        const uint32_t tw = (uint32_t)fd.tile_w, th = (uint32_t)fd.tile_h, tiles_x = (P.gw + tw - 1u) / tw;
        ty0 = P.row0 / th;
        tile_rows = P.row1 > P.row0 ? (P.row1 - 1u) / th - ty0 + 1u : 0u;
        per_row = (tiles_x + (uint32_t)fd.world - 1u) / (uint32_t)fd.world;
        tile_lis = tw * th;
        count = tile_rows * per_row * tile_lis * P.spp;
    }
    // entry v -> launch index (lx, ly) and sample s; false: the entry is padding (a tile beyond the row's end, a launch index
    // beyond the grid or outside the job's rows)
    __device__ inline bool at(const FrameDev& fd, const PassDev& P, uint32_t v, uint32_t& lx, uint32_t& ly, uint32_t& s) const
    {
        const uint32_t tw = (uint32_t)fd.tile_w, th = (uint32_t)fd.tile_h, world = (uint32_t)fd.world;
        const uint32_t t = v / P.spp;
        s = v - t * P.spp;
        const uint32_t tile = t / tile_lis, in = t - tile * tile_lis;
        const uint32_t row = tile / per_row, k = tile - row * per_row;
        const uint32_t ty = ty0 + row;
        const uint32_t first = ((uint32_t)fd.rank + world - (3u * ty + P.frame_pass) % world) % world;    // (tx + 3 ty + pass) % world == rank
        const uint32_t tx = first + k * world;
        const uint32_t iy = in / tw;
        lx = tx * tw + (in - iy * tw);
        ly = ty * th + iy;
        return lx < P.gw && ly >= P.row0 && ly < P.row1;
    }
};

// One block iteration of the generate kernels: the camera rays of its live threads (launch index (lx, ly) of pass P, sample s,
// sample slot `slot`, pixel (ix, iy) from ring_alive) and their append to queue 0.  Called by every thread of the block.
__device__ inline void generate_rays(const FrameDev& fd, const PathState& ps, const RayQueue& queue0, uint32_t cap, Counters* __restrict__ cnt,
                                     uint32_t* s_scratch, uint32_t sel, const PassDev& P, bool live, uint32_t slot, uint32_t lx, uint32_t ly,
                                     uint32_t s, uint32_t ix, uint32_t iy)
{
    V3 ray_dir = v3(0.f);
    if (live) {
        uint32_t seed = tea4(ly * (uint32_t)fd.w + lx, P.subframe);        // :411
        for (uint32_t k = 0; k < s; k++) { (void)rnd(seed); (void)rnd(seed); }   // earlier samples' jitter draws
        Rng rng;                                                            // Random(seed), maths.h:176-180
        rng.s1 = 315645664u + seed;
        rng.s2 = rng.s1 ^ 0x13ab45feu;
        const float jx = rnd(seed);                                         // :479, x first
        const float jy = rnd(seed);
        const float dx = 2.0f * (((float)ix + jx) / (float)fd.w) - 1.0f;    // :483-486
        const float dy = 2.0f * (((float)iy + jy) / (float)fd.h) - 1.0f;
        const V3 U = v3(fd.U[0], fd.U[1], fd.U[2]), V = v3(fd.V[0], fd.V[1], fd.V[2]), W = v3(fd.W[0], fd.W[1], fd.W[2]);
        const V3 dir = normalize(dx * U + dy * V + W);                      // :491
        ray_dir = dir;
        st_stream<FOVPT_STREAM_STATE>(ps.rng + slot, make_uint4(rng.s1, rng.s2, 0u, 0u));     // stateFlags 0, depth 0
        // Nothing else is initialised: pathThroughput / rayEta are (1,1,1) / 1 until the first shaded hit
        // (k_shade), the radiance cells [0, depth) and alpha are written exactly once before resolve
        // reads them (depth and FLAG_ALPHA_SET tell it which), :450-451
        if (ps.guide_n) {
            st_stream<FOVPT_STREAM_CELLS>(ps.guide_n + slot, make_float4(0.f, 0.f, 0.f, 0.f));
            st_stream<FOVPT_STREAM_CELLS>(ps.guide_a + slot, make_float4(0.f, 0.f, 0.f, 0.f));
        }
        if (s == P.spp - 1) {                                               // backplate of the last sample, :495
            float u, v;
            probe_dir_to_uv(dir, u, v);
            st_stream<FOVPT_STREAM_CELLS>(ps.backplate + (P.launch_base + (ly - P.row0) * P.gw + lx), probe_eval(fd.probe, fd.probe_row_mul, u, v));
        }
    }
    const uint32_t pos = block_append(cnt, FOVPT_CNT_Q(0), cap, live, s_scratch, sel);
    if (live) {
        st_stream<FOVPT_STREAM_RAYQ>(queue0.o + pos, make_float4(fd.eye[0], fd.eye[1], fd.eye[2], __uint_as_float(slot)));
        st_stream<FOVPT_STREAM_RAYQ>(queue0.d + pos, f4(ray_dir, 0.f));
    }
}

__global__ __launch_bounds__(FOVPT_BLOCK) void k_generate(const FrameDev fd, PathState ps, RayQueue queue0, uint32_t cap,
                                                          Counters* __restrict__ cnt, uint32_t slot_begin, uint32_t total_slots, uint32_t sel)
{
    // slots [slot_begin, total_slots) into the shards of `sel` (a whole job: 0 .. all slots, all shards; a chain: its half)
    __shared__ uint32_t s_scratch[6];
    for (uint32_t base = slot_begin + blockIdx.x * FOVPT_BLOCK; base < total_slots; base += gridDim.x * FOVPT_BLOCK) {
        const uint32_t slot = base + threadIdx.x;
        bool live = slot < total_slots;
        int p = 0;
        uint32_t lx = 0, ly = 0, s = 0, ix = 0, iy = 0;
        if (live) {
            while (p + 1 < fd.npass && slot >= fd.pass[p + 1].slot_base) p++;
            const PassDev& P = fd.pass[p];
            const uint32_t rel = slot - P.slot_base;
            const uint32_t li = rel / P.spp;
            s = rel - li * P.spp;
            ly = li / P.gw;
            lx = li - ly * P.gw;
            ly += P.row0;                                      // slots and launch records are relative to the chunk
            live = ring_alive(fd, P, lx, ly, ix, iy) && launch_owned(fd, p, lx, ly);
        }
        generate_rays(fd, ps, queue0, cap, cnt, s_scratch, sel, fd.pass[p], live, slot, lx, ly, s, ix, iy);
    }
}

// The same for a rank of a tile-sharded frame (world > 1, one chain): the grid walks the rank's own tiles, see OwnedSpace -- every
// pass padded to whole block iterations, so that a block iteration serves ONE pass and reads its record with scalar loads.
__global__ __launch_bounds__(FOVPT_BLOCK) void k_generate_owned(const FrameDev fd, PathState ps, RayQueue queue0, uint32_t cap,
                                                                Counters* __restrict__ cnt)
{
    __shared__ uint32_t s_scratch[6];
    static_assert(FOVPT_MAX_PASSES == 3, "the pass of a block iteration is selected by hand below");
    OwnedSpace o0, o1, o2;
    o0.count = o1.count = o2.count = 0u;
    if (fd.npass > 0) o0.init(fd, fd.pass[0]);
    if (fd.npass > 1) o1.init(fd, fd.pass[1]);
    if (fd.npass > 2) o2.init(fd, fd.pass[2]);
    const uint32_t b0 = (o0.count + FOVPT_BLOCK - 1u) / FOVPT_BLOCK, b1 = (o1.count + FOVPT_BLOCK - 1u) / FOVPT_BLOCK,
                   b2 = (o2.count + FOVPT_BLOCK - 1u) / FOVPT_BLOCK;
    for (uint32_t it = blockIdx.x; it < b0 + b1 + b2; it += gridDim.x) {
        const int p = it < b0 ? 0 : it < b0 + b1 ? 1 : 2;
        const OwnedSpace own = p == 0 ? o0 : p == 1 ? o1 : o2;
        const PassDev& P = fd.pass[p];
        const uint32_t v = (it - (p == 0 ? 0u : p == 1 ? b0 : b0 + b1)) * FOVPT_BLOCK + threadIdx.x;
        uint32_t lx = 0, ly = 0, s = 0, ix = 0, iy = 0;
        bool live = v < own.count && own.at(fd, P, v, lx, ly, s);
        const uint32_t slot = P.slot_base + ((ly - P.row0) * P.gw + lx) * P.spp + s;
        live = live && ring_alive(fd, P, lx, ly, ix, iy) && launch_owned(fd, p, lx, ly);
        generate_rays(fd, ps, queue0, cap, cnt, s_scratch, 0u, P, live, slot, lx, ly, s, ix, iy);
    }
}

// ---- shade -------------------------------------------------------------------------------
#define FLAG_DONE 1u
#define FLAG_SECONDARY 2u

#define FLAG_ALPHA_ONE 4u      // prd.alpha = make_float3(1) happened (deviceProgram.cu:689)
#define FLAG_ALPHA_SET 8u      // prd.alpha += ... happened on a shadow catcher (:693): ps.alpha[slot] holds it

#ifndef FOVPT_V_SHADEWAVES
#define FOVPT_V_SHADEWAVES 1
#endif
// EXTRA: the build of the kernel that also knows the opt-in extensions of fovpt_config.options (sky radiance for escaped
// secondary rays, Russian roulette); the default build carries none of their code or registers.
template <bool EXTRA>
__global__ __launch_bounds__(FOVPT_BLOCK, FOVPT_V_SHADEWAVES) void k_shade(const FrameDev fd, SceneView sc, PathState ps,
                                                       RayQueue queue_in, RayQueue queue_out,
                                                       ShadowQueue sq, uint32_t cap, Counters* __restrict__ cnt, int depth_iter, uint32_t sel)
{
    __shared__ uint32_t s_scratch[14];
    ShardMap mq;
    mq.load(cnt, FOVPT_CNT_Q(depth_iter), sel, cap);
    const uint32_t n = mq.total();
    const uint32_t nround = (n + FOVPT_BLOCK - 1) / FOVPT_BLOCK * FOVPT_BLOCK;
    for (uint32_t i = blockIdx.x * FOVPT_BLOCK + threadIdx.x; i < nround; i += gridDim.x * FOVPT_BLOCK) {
        bool want_shadow = false, want_next = false;
        uint32_t slot = 0;
        V3 next_o = v3(0.f), next_d = v3(0.f);
        float next_pdf = 0.f;          // prd.bsdfPdf of the sample that sends the next ray (read by FOVPT_OPT_SKY_MISS only)
        float4 sh_o, sh_d, sh_vis, sh_occ;
        sh_o = sh_d = sh_vis = sh_occ = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < n) {
            const uint32_t ph = mq.phys(i, cap);
            const float4 o4 = ld_stream<FOVPT_STREAM_RAYQ>(queue_in.o + ph), d4 = ld_stream<FOVPT_STREAM_RAYQ>(queue_in.d + ph);
            slot = __float_as_uint(o4.w);
            const float4 hit = ld_stream<FOVPT_STREAM_HIT>(ps.hit + ph);
            const uint32_t tpos = __float_as_uint(hit.w);
            uint4 rs = ld_stream<FOVPT_STREAM_STATE>(ps.rng + slot);
            uint32_t flags = rs.z & 0xffu;
            int depth = (int)(rs.z >> 8);
            if (tpos == 0xffffffffu) {
                // __miss__radiance :253-282: DONE; nothing is added for this segment (:515 breaks first)
                flags |= FLAG_DONE;
                if (EXTRA && (fd.options & FOVPT_OPT_SKY_MISS) && (flags & FLAG_SECONDARY) && depth < fd.max_depth) {
                    // the block the reference carries commented out (:259-269): MIS counterpart of SampleLights; the
                    // segment is counted (one more radiance cell), see include/fovpt.h
                    const V3 dir = v3(d4);
                    const float bsdfPdf = d4.w;                                            // pdf of the sample that sent this ray
                    const V3 thr = v3(ld_stream<FOVPT_STREAM_STATE>(ps.thr + slot));
                    float u, v;
                    probe_dir_to_uv(dir, u, v);
                    const fovpt_probe& pr = fd.probe;                                      // ProbePdf, Probe.cuh:69-93
                    const int col = max(0, min((int)(u * pr.width), pr.width - 1));
                    const int row = max(0, min((int)(v * pr.height), pr.height - 1));
                    float skyPdf = pr.pdfValuesX[row * fd.probe_row_mul * pr.width + col] * pr.pdfValuesY[row];
                    const float sinTheta = fovpt_dm_sinf(v * kPi);
                    if (fabsf(sinTheta) < 0.0001f) skyPdf = 0.0f;
                    else skyPdf *= float(pr.width) * float(pr.height) / (2.0f * kPi * kPi * sinTheta);
                    const float weight = 0.5f * bsdfPdf / (0.5f * bsdfPdf + 0.5f * skyPdf);
                    const V3 rad = v3(0.f) + (weight * v3(probe_eval(pr, fd.probe_row_mul, u, v))) * thr;
                    st_stream<FOVPT_STREAM_CELLS>(ps.rad + ((size_t)slot * ps.stride + depth), f4(rad, 0.f));
                    depth += 1;
                }
            } else {
                const V3 ray_o = v3(o4), ray_dir = v3(d4);
                // ProbeSample is the first consumer of the path's random numbers on a shaded hit (:303-344) and
                // depends on nothing else: its chain of dependent loads (guide tables, CDFs, texel) is started
                // here, beside the chain hit -> triangle -> mesh -> texels.  Branches that do not shade drop it.
                Rng rng_probe; rng_probe.s1 = rs.x; rng_probe.s2 = rs.y;
                V3 wi, skyColor; float skyPdf;
                probe_sample(fd.probe, fd.guide_x, fd.guide_y, fd.probe_rec, fd.probe_row_mul, wi, skyColor, skyPdf, rng_probe);
                const float4 thr_in = ld_stream<FOVPT_STREAM_STATE>(ps.thr + slot);      // (unused garbage until the first shaded hit wrote it)
                const TriRec T = load_tri_off(sc.tris, tpos << 4);            // tpos: offset in 16-byte units
                const MeshDev M = sc.meshes[T.mesh];
                const Mat& mat = M.material;
                const V3 e1 = v3(T.e1x, T.e1y, T.e1z), e2 = v3(T.e2x, T.e2y, T.e2z);
                const V3 N_0 = normalize(cross(e1, e2));                                   // :632
                const V3 wo = neg(ray_dir);
                const V3 N = N_0 * copysignf(1.0f, dot(wo, N_0));                          // faceforward :634
                const V3 P = ray_o + hit.x * ray_dir;                                      // :638
                const bool catcher = (mat.flags & FOVPT_MATERIAL_FLAG_SHADOW_CATCHER) != 0;
                if (catcher && (flags & FLAG_SECONDARY)) {
                    // :646-651: pass straight through, depth unchanged after the loop's ++depth;
                    // the loop adds prd.radiance == 0 to direct/indirect, which changes nothing
                    next_o = P; next_d = ray_dir; next_pdf = d4.w;
                    want_next = true;
                } else if (depth >= fd.max_depth) {
                    // the reference's discarded last segment (:515).  It is only traced here when the
                    // scene holds a shadow catcher; a catcher hit is always a pass-through at this
                    // depth (SECONDARY is set), so this is a plain hit whose one lasting effect is :689
                    flags |= FLAG_ALPHA_ONE | FLAG_DONE;
                } else {
                    // pathThroughput (1,1,1) and rayEta 1 until the first shaded hit (:447-449)
                    const float4 t4 = (flags & FLAG_SECONDARY) ? thr_in : make_float4(1.f, 1.f, 1.f, 1.0f);
                    V3 thr = v3(t4);
                    float rayEta = t4.w;
                    Rng rng = rng_probe;
                    V3 albedo = v3(mat.color);
                    if (M.texture_id >= 0 && M.has_texcoord) {                             // :655-670
                        const float2* tc = sc.tri_tc + (size_t)T.prim * 3;
                        const float2 t0 = tc[0], t1 = tc[1], t2 = tc[2];
                        const float w0 = 1.f - hit.y - hit.z;
                        const float tcx = (w0 * t0.x + hit.y * t1.x) + hit.z * t2.x;
                        const float tcy = (w0 * t0.y + hit.y * t1.y) + hit.z * t2.y;
                        albedo = v3(tex2d(M.tex, tcx, tcy));
                    }
                    if (ps.guide_n && depth == 0 && (flags & FLAG_SECONDARY) == 0) {       // :509-512, :653-654
                        st_stream<FOVPT_STREAM_CELLS>(ps.guide_n + slot, f4(N, 0.f));
                        st_stream<FOVPT_STREAM_CELLS>(ps.guide_a + slot, f4(albedo, 0.f));
                    }
                    float outEta;
                    if (rayEta == 1.0f)                                                    // :673-683
                        outEta = (mat.eta == 0.0f) ? 2.0f / (1.0f - sqrtf(0.08f * mat.specular)) - 1.0f : mat.eta;
                    else
                        outEta = 1.0f;
                    // ---- SampleLights / SampleShadow :303-387 with the occlusion test deferred
                    const BsdfView view = bsdf_view(mat, albedo, rayEta, outEta, N, wo);
                    V3 sum_hit = v3(0.0f);        // value of `sum` on the branch that evaluates the BSDF
                    {
                        const float bsdfPdf = bsdf_pdf(mat, view, N, wo, wi);
                        const V3 f = bsdf_eval(mat, albedo, view, N, wo, wi);
                        if (bsdfPdf > 0.0f) {
                            const float weight = 0.5f * skyPdf / (0.5f * bsdfPdf + 0.5f * skyPdf);
                            if (weight > 0.0f) {
                                const V3 val = div_vs(weight * skyColor * f * fabsf(dot(wi, N)), skyPdf) * (1.0f / 1.f);
                                sum_hit = sum_hit + val;
                            }
                        }
                    }
                    const V3 sum_zero = v3(0.0f);
                    V3 rad_vis, rad_occ;          // prd.radiance after this hit if the shadow ray is un/occluded
                    V3 alpha_vis = v3(0.f), alpha_occ = v3(0.f);
                    bool alpha_set_one = false;
                    if (!catcher) {                                                        // :686-690
                        rad_vis = v3(0.f) + thr * sum_hit;
                        rad_occ = v3(0.f) + thr * sum_zero;
                        alpha_set_one = true;
                    } else {                                                               // :691-694 SampleShadow
                        rad_vis = v3(0.f); rad_occ = v3(0.f);
                        alpha_vis = thr * sum_zero;
                        alpha_occ = thr * sum_hit;
                    }
                    if ((flags & FLAG_SECONDARY) == 0) {                                   // :696-698
                        rad_vis = rad_vis + v3(mat.emission);
                        rad_occ = rad_occ + v3(mat.emission);
                    }
                    V3 bu, bv;
                    basis_from_vector(N, bu, bv);
                    V3 bsdfDir = v3(0.f);
                    const float bsdfPdf = bsdf_sample(mat, view, bu, bv, N, wo, bsdfDir, rng);            // :706
                    if (alpha_set_one) flags |= FLAG_ALPHA_ONE;                            // :689 (kept even when DONE)
                    const bool same = rad_vis.x == rad_occ.x && rad_vis.y == rad_occ.y && rad_vis.z == rad_occ.z
                                   && alpha_vis.x == alpha_occ.x && alpha_vis.y == alpha_occ.y && alpha_vis.z == alpha_occ.z;
                    if (catcher) {
                        // alpha += thr * shadowSample happens regardless of what follows (:693); alpha is still
                        // (0,0,0) here because only a primary hit gets this far on a catcher
                        flags |= FLAG_ALPHA_SET;
                        if (same) st_stream<FOVPT_STREAM_CELLS>(ps.alpha + slot, f4(v3(0.f) + alpha_occ, 0.f));
                        else {
                            want_shadow = true;
                            sh_o = f4(P, __uint_as_float(slot)); sh_d = f4(wi, __uint_as_float(0xffffffffu));
                            sh_vis = f4(v3(0.f) + alpha_vis, 0.f); sh_occ = f4(v3(0.f) + alpha_occ, 0.f);
                        }
                    }
                    if (bsdfPdf <= 0.0f) {                                                 // :708-711
                        flags |= FLAG_DONE;       // radiance of this hit is dropped by the break at :515
                    } else {
                        // the segment counts: prd.radiance becomes the depth-th term of directLight (depth 0) /
                        // indirectLight (:522-527).  One cell per (slot, depth), summed in order by resolve.
                        float4* cell = ps.rad + ((size_t)slot * ps.stride + depth);
                        if (!catcher && !same) {
                            want_shadow = true;
                            sh_o = f4(P, __uint_as_float(slot)); sh_d = f4(wi, __uint_as_float((uint32_t)depth));
                            sh_vis = f4(rad_vis, 0.f); sh_occ = f4(rad_occ, 0.f);
                        } else {
                            st_stream<FOVPT_STREAM_CELLS>(cell, f4(rad_occ, 0.f));
                        }
                        flags |= FLAG_SECONDARY;
                        depth += 1;                                                        // :529
                        // The reference traces once more at depth == max_depth and throws the result
                        // away (:515).  Without a shadow catcher in the scene that segment cannot
                        // change anything (alpha is already 1), so it is not traced -- and then nothing reads the
                        // throughput, the medium or the random numbers of this path any more (:714-724 skipped).
                        if (depth < fd.max_depth || sc.any_catcher) {
                            const V3 f = bsdf_eval(mat, albedo, view, N, wo, bsdfDir);              // :714
                            if (dot(bsdfDir, N) <= 0.0f) rayEta = outEta;                  // :717-721
                            thr = thr * div_vs(f * fabsf(dot(N, bsdfDir)), bsdfPdf);       // :724
                            bool rr_kill = false;
                            if (EXTRA && (fd.options & FOVPT_OPT_RUSSIAN_ROULETTE) && depth >= 2) {   // the //!TODO of :518-520, see include/fovpt.h
                                const float q = fmaxf(0.05f, fminf(1.0f, fmaxf(thr.x, fmaxf(thr.y, thr.z))));
                                if (rng.randf() >= q) rr_kill = true;
                                else thr = thr * (1.0f / q);
                            }
                            if (!rr_kill) {
                                next_o = P; next_d = bsdfDir; next_pdf = bsdfPdf;
                                st_stream<FOVPT_STREAM_STATE>(ps.thr + slot, f4(thr, rayEta));
                                want_next = true;
                            }
                        }
                    }
                    rs.x = rng.s1; rs.y = rng.s2;
                }
            }
            rs.z = flags | ((uint32_t)depth << 8);
            st_stream<FOVPT_STREAM_STATE>(ps.rng + slot, rs);
        }
        // ---- wavefront-ballot compaction into the next queues
        uint32_t spos, qpos;
        if (fd.partition)                                                          // (block-uniform)
            block_append2d(cnt, FOVPT_CNT_SQ(depth_iter), want_shadow, FOVPT_CNT_Q(depth_iter + 1), want_next, next_d.y > 0.0f, cap, s_scratch, spos, qpos, sel);
        else
            block_append2(cnt, FOVPT_CNT_SQ(depth_iter), want_shadow, FOVPT_CNT_Q(depth_iter + 1), want_next, cap, s_scratch, spos, qpos, sel);
        if (want_shadow) {
            st_stream<FOVPT_STREAM_SHADOWQ>(sq.o + spos, sh_o); st_stream<FOVPT_STREAM_SHADOWQ>(sq.d + spos, sh_d);
            st_stream<FOVPT_STREAM_SHADOWQ>(sq.val_vis + spos, sh_vis); st_stream<FOVPT_STREAM_SHADOWQ>(sq.val_occ + spos, sh_occ);
        }
        if (want_next) {
            st_stream<FOVPT_STREAM_RAYQ>(queue_out.o + qpos, f4(next_o, __uint_as_float(slot)));
            st_stream<FOVPT_STREAM_RAYQ>(queue_out.d + qpos, f4(next_d, next_pdf));
        }
    }
}

// ---- resolve -----------------------------------------------------------------------------
// Resolve as a tiled LDS reduction.  A block owns a 64 x 4 pixel tile.
//   A. every pixel thread finds its last writer in the reference's launch order (gather)
//   B. runs of pixels with the same writer elect a leader; leaders are ballot-compacted into a tile-local
//      work list in LDS (a 4x4 periphery block is 16 pixels but ONE colour)
//   C. the first n threads of the block each reduce one list entry: ordered sum over the launch index's
//      sample slots and bounce cells, alpha, backplate mix, exposure, Reinhard, sRGB -> LDS
//   D. every pixel thread fetches its colour from LDS and writes float4 accum + rgba8, coalesced
//   E. (block 0) the job's queue counters are zeroed for the next job that uses this state set: resolve
//      is the last kernel of a job and nothing in it reads them
__global__ __launch_bounds__(FOVPT_BLOCK) void k_resolve(const FrameDev fd, PathState ps, Counters* __restrict__ cnt)
{
    if (!FOVPT_V_STEPSTAT && blockIdx.x == 0 && blockIdx.y == 0) {     // (a diagnostic build keeps them for tools/raystat.py)
        uint32_t* w = &cnt->shard[0][0];
        for (uint32_t i = threadIdx.x; i < FOVPT_SHARDS * FOVPT_SHARD_STRIDE; i += FOVPT_BLOCK) w[i] = 0u;
    }
    __shared__ uint32_t s_key[FOVPT_BLOCK];        // launch record id of the pixel's writer
    __shared__ uint32_t s_idx[FOVPT_BLOCK];        // leader thread -> tile list position
    __shared__ uint32_t s_list_li[FOVPT_BLOCK];    // tile list: launch index ...
    __shared__ uint32_t s_list_p[FOVPT_BLOCK];     // ... and pass
    __shared__ float4 s_accum[FOVPT_BLOCK];        // result per list entry: accum_color (pre-blend)
    __shared__ uint32_t s_rgba[FOVPT_BLOCK];       // result per list entry: tone-mapped pixel
    __shared__ float4 s_gn[FOVPT_BLOCK], s_ga[FOVPT_BLOCK];   // denoiser guides per list entry
    __shared__ uint32_t s_wave[4];

    const uint32_t tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const uint32_t x = blockIdx.x * 64 + tx;
    const uint32_t y = blockIdx.y * 4 + ty;
    const bool inside = x < (uint32_t)fd.w && y < (uint32_t)fd.h;
    const uint32_t image_index = y * (uint32_t)fd.w + x;

    // ---- A: last writer of this pixel
    int state = 0;                 // 0 nobody, 1 a launch index this rank owns, 2 another rank's
    int wp = 0;
    uint32_t wli = 0, key = 0xffffffffu;
    if (inside) {
        uint32_t wlx, wly;
        if (find_last_writer(fd, x, y, wp, wlx, wly)) {
            const PassDev& P = fd.pass[wp];
            state = launch_owned(fd, wp, wlx, wly) ? 1 : 2;
            wli = (wly - P.row0) * P.gw + wlx;
            key = P.launch_base + wli;
        }
    }
    if (state != 1) key = 0xffffffffu;
    s_key[threadIdx.x] = key;
    __syncthreads();

    // ---- B: run leaders -> tile list
    const bool leader = state == 1 && (tx == 0 || s_key[threadIdx.x - 1] != key);
    const unsigned long long lm = __ballot(leader);
    if (tx == 0) s_wave[ty] = (uint32_t)__popcll(lm);
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t w = 0; w < ty; w++) base += s_wave[w];
    const uint32_t nlist = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    if (leader) {
        const uint32_t pos = base + (uint32_t)__popcll(lm & ((1ull << tx) - 1ull));
        s_idx[threadIdx.x] = pos;
        s_list_li[pos] = wli;
        s_list_p[pos] = (uint32_t)wp;
    }
    __syncthreads();

    // ---- C: one thread per distinct writer in the tile
    if (threadIdx.x < nlist) {
        const PassDev& P = fd.pass[s_list_p[threadIdx.x]];
        const uint32_t li = s_list_li[threadIdx.x];
        const uint32_t s0 = P.slot_base + li * P.spp;
        V3 result = v3(0.0f), alpha = v3(0.0f), gnorm = v3(0.0f), galb = v3(0.0f);
        for (uint32_t s = 0; s < P.spp; s++) {                                     // :536-537, in sample order
            const uint32_t slot = s0 + s;
            if (ps.guide_n) { gnorm = gnorm + v3(ld_stream<FOVPT_STREAM_CELLS>(ps.guide_n + slot)); galb = galb + v3(ld_stream<FOVPT_STREAM_CELLS>(ps.guide_a + slot)); }   // :510-511
            const float4* cells = ps.rad + (size_t)slot * ps.stride;                 // one 16*D-byte record per slot
            // the path's `depth` segments counted, cell dd holds prd.radiance of segment dd; the reference
            // adds nothing for a segment it never reached
            const uint32_t st = ld_stream<FOVPT_STREAM_STATE>(&ps.rng[slot].z);
            const int nseg = min((int)(st >> 8), fd.max_depth);
            const V3 direct = v3(0.0f) + (nseg > 0 ? v3(ld_stream<FOVPT_STREAM_CELLS>(cells)) : v3(0.0f));          // :523
            V3 indirect = v3(0.0f);
            for (int dd = 1; dd < nseg; dd++)                                          // :526, in bounce order
                indirect = indirect + v3(ld_stream<FOVPT_STREAM_CELLS>(cells + dd));
            result = result + (direct + indirect);
            alpha = alpha + ((st & FLAG_ALPHA_ONE) ? v3(1.0f) : (st & FLAG_ALPHA_SET) ? v3(ld_stream<FOVPT_STREAM_CELLS>(ps.alpha + slot)) : v3(0.0f));
        }
        const float sppf = (float)P.spp;
        { const float inv = 1.0f / sppf; alpha = alpha * inv; gnorm = gnorm * inv; galb = galb * inv; }   // :541-543
        const V3 backplate = v3(ld_stream<FOVPT_STREAM_CELLS>(ps.backplate + (P.launch_base + li)));
        const V3 color = (backplate * sppf) * sub_sv(1.0f, alpha) + result;        // :558
        const V3 accum_color = div_vs(color, sppf);                                // :560
        s_gn[threadIdx.x] = f4(gnorm, 1.0f); s_ga[threadIdx.x] = f4(galb, 1.0f);
        s_accum[threadIdx.x] = f4(accum_color, 1.0f);
        s_rgba[threadIdx.x] = make_color(reinhard(accum_color * 16.0f, 1.0f));     // :586,597
    }
    __syncthreads();

    // ---- D: write the tile
    if (!inside) return;
    if (state == 1) {
        uint32_t t = threadIdx.x;
        while (!(t == ty * 64 || s_key[t - 1] != key)) t--;                        // start of this pixel's run
        const uint32_t e = s_idx[t];
        const PassDev& P = fd.pass[wp];
        float4 a = s_accum[e];
        uint32_t rgba = s_rgba[e];
        if (fd.accumulate && P.subframe > 0 && !P.redraw) {
            // PT_sv4_vmv2/deviceProgram.cu:545-553: clamp + running mean against THIS pixel's history
            V3 accum_color = clamp3(v3(a), 0.0f, 10.0f);
            const float alpha_value = 1.0f / (float)(P.subframe + 1);
            const fovpt_float4 pv = fd.accum_prev[image_index];
            accum_color = lerp3(v3(pv.x, pv.y, pv.z), accum_color, alpha_value);
            a = f4(accum_color, 1.0f);
            rgba = make_color(reinhard(accum_color * 16.0f, 1.0f));
        }
        fd.accum[image_index] = fovpt_float4{a.x, a.y, a.z, 1.0f};                 // :582
        fd.frame[image_index] = rgba;
        if (ps.guide_n) {                                                          // :612-614
            const float4 gn = s_gn[e], ga = s_ga[e];
            if (fd.g_normal) fd.g_normal[image_index] = fovpt_float4{gn.x, gn.y, gn.z, 1.0f};
            if (fd.g_color) fd.g_color[image_index] = fovpt_float4{a.x, a.y, a.z, 1.0f};
            if (fd.g_albedo) fd.g_albedo[image_index] = fovpt_float4{ga.x, ga.y, ga.z, 1.0f};
        }
    } else if (state == 2 || fd.zero_holes) {
        // another rank's pixel (or, for a whole frame on a rank other than 0, nobody's): zero keeps the sum-gather exact
        fd.accum[image_index] = fovpt_float4{0.f, 0.f, 0.f, 0.f};
        fd.frame[image_index] = 0u;
    }
}

// ---- multi-GPU: packed gather of the owned pixels -------------------------------------------------
// Every pixel of a frame has one last writer (find_last_writer) and that launch index has one owning rank
// (launch_owned: interleaved 8x4 launch-index tiles, the scheme of sutil/WorkDistribution.h:47-84), so the pixels of a
// frame partition by owner.  The PLAN lists, rank by rank, the pixel indices a rank owns in ascending order; every rank
// builds the same plan from the same launch parameters.  Per frame a rank packs its owned rgba8 words into a contiguous
// buffer (k_gather_pack), RCCL gathers the buffers onto rank 0, and rank 0 scatters them into the frame
// (k_gather_unpack): 1/N of the bytes of a full-frame reduce per rank.
#define FOVPT_PLAN_NOBODY 255u
__device__ inline uint32_t launch_owner_rank(const FrameDev& fd, int p, uint32_t lx, uint32_t ly)
{
    if (fd.world <= 1) return 0u;
    const uint32_t tx = lx / (uint32_t)fd.tile_w, ty = ly / (uint32_t)fd.tile_h;
    return (tx + 3u * ty + fd.pass[p].frame_pass) % (uint32_t)fd.world;
}
// owner[pixel] and, per block of 256 consecutive pixels, the number of pixels every rank owns
__global__ __launch_bounds__(FOVPT_BLOCK) void k_plan_owner(const FrameDev fd, uint8_t* __restrict__ owner, uint32_t* __restrict__ block_count)
{
    __shared__ uint32_t s_cnt[64];
    if (threadIdx.x < 64) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t npix = (uint32_t)fd.w * (uint32_t)fd.h;
    const uint32_t i = blockIdx.x * FOVPT_BLOCK + threadIdx.x;
    uint32_t o = FOVPT_PLAN_NOBODY;
    if (i < npix) {
        const uint32_t y = i / (uint32_t)fd.w, x = i - y * (uint32_t)fd.w;
        int wp; uint32_t lx, ly;
        if (find_last_writer(fd, x, y, wp, lx, ly)) o = launch_owner_rank(fd, wp, lx, ly);
        owner[i] = (uint8_t)o;
    }
    if (o != FOVPT_PLAN_NOBODY) atomicAdd(&s_cnt[o], 1u);
    __syncthreads();
    if ((int)threadIdx.x < fd.world) block_count[(size_t)blockIdx.x * fd.world + threadIdx.x] = s_cnt[threadIdx.x];
}
// exclusive scan of the block counts, rank by rank: ONE BLOCK per rank, every thread scans a contiguous chunk of the counts,
// the chunk totals are scanned in LDS, the chunks are written back with their offsets.  (The plan is rebuilt whenever the gaze
// moves -- every frame with an eye tracker -- so this is not a one-off: a single thread per rank walking 8-18 k blocks was.)
__global__ __launch_bounds__(1024) void k_plan_scan(uint32_t nblocks, int world, uint32_t* __restrict__ block_count, uint32_t* __restrict__ total)
{
    __shared__ uint32_t s_part[1024];
    const int r = (int)blockIdx.x;
    if (r >= world) return;
    const uint32_t per = (nblocks + blockDim.x - 1u) / blockDim.x;
    const uint32_t b0 = min(nblocks, threadIdx.x * per), b1 = min(nblocks, b0 + per);
    uint32_t sum = 0u;
    for (uint32_t b = b0; b < b1; b++) sum += block_count[(size_t)b * world + r];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t off = 1u; off < blockDim.x; off <<= 1) {                    // inclusive Hillis-Steele scan of the chunk totals
        const uint32_t v = threadIdx.x >= off ? s_part[threadIdx.x - off] : 0u;
        __syncthreads();
        s_part[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = s_part[threadIdx.x] - sum;                                   // exclusive offset of my chunk
    for (uint32_t b = b0; b < b1; b++) {
        const uint32_t c = block_count[(size_t)b * world + r];
        block_count[(size_t)b * world + r] = run;
        run += c;
    }
    if (threadIdx.x == blockDim.x - 1u) total[r] = s_part[threadIdx.x];
}
// idx[rank_base[o] + block offset + position among the block's pixels of the same owner] = pixel
__global__ __launch_bounds__(FOVPT_BLOCK) void k_plan_fill(uint32_t npix, int world, const uint8_t* __restrict__ owner, const uint32_t* __restrict__ block_off,
                                                          const uint32_t* __restrict__ rank_base, uint32_t* __restrict__ idx)
{
    // position of a pixel among the block's pixels of the same owner, in ascending pixel order: within a wave one ballot per
    // DISTINCT owner present (64 consecutive pixels span a handful of 8-pixel-wide tiles), the waves' counts meet in LDS.
    // (Was: every thread scanning the up to 255 owners before it.)
    __shared__ uint32_t s_cnt[FOVPT_BLOCK / 64][64];
    const uint32_t i = blockIdx.x * FOVPT_BLOCK + threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t o = i < npix ? owner[i] : FOVPT_PLAN_NOBODY;
    for (uint32_t k = threadIdx.x; k < (FOVPT_BLOCK / 64) * 64; k += FOVPT_BLOCK) (&s_cnt[0][0])[k] = 0u;
    __syncthreads();
    uint32_t in_wave = 0u;
    unsigned long long todo = __ballot(o != FOVPT_PLAN_NOBODY);
    while (todo) {                                                             // wave-uniform loop over the owners present
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)o, (int)leader);
        const unsigned long long same = __ballot(o == lo);
        if (o == lo) in_wave = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        if (lane == leader) s_cnt[wave][lo] = (uint32_t)__popcll(same);
        todo &= ~same;
    }
    __syncthreads();
    if (o == FOVPT_PLAN_NOBODY) return;
    uint32_t before = in_wave;
    for (uint32_t w = 0; w < wave; w++) before += s_cnt[w][o];
    idx[rank_base[o] + block_off[(size_t)blockIdx.x * world + o] + before] = i;
}
__global__ void k_gather_pack(uint32_t n, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ frame, uint32_t* __restrict__ packed)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) packed[i] = frame[idx[i]];
}
// gathered: `world` buffers of `stride` words; rank r's pixels are idx[base[r] .. base[r+1])
__global__ void k_gather_unpack(int world, uint32_t stride, const uint32_t* __restrict__ base, const uint32_t* __restrict__ idx,
                                const uint32_t* __restrict__ gathered, uint32_t* __restrict__ frame)
{
    const uint32_t total = base[world];
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        int r = 0;
        while (r + 1 < world && i >= base[r + 1]) r++;
        frame[idx[i]] = gathered[(size_t)r * stride + (i - base[r])];
    }
}

// ---- probe guide tables (built once per setProbe) ------------------------------------------
// guide[seg * (n+2) + m] = lower_bound(cdf[seg*n .. seg*n+n), fl(m * fl(1/n))) - seg*n, m = 0..n+1
__global__ void k_build_guide(const float* __restrict__ cdf, int n, int segments, uint32_t* __restrict__ guide)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)segments * (n + 2);
    if (i >= total) return;
    const int seg = (int)(i / (n + 2)), m = (int)(i - (size_t)seg * (n + 2));
    const float value = (float)m * (1.0f / (float)n);                 // w_m of lower_bound_guided
    guide[i] = (uint32_t)(lower_bound(cdf, seg * n, (seg + 1) * n, value) - seg * n);
}

// packed per-texel records for probe_sample: {cdfX, pdfX, r, g, b, 0, 0, 0}
__global__ void k_probe_records(size_t n, const float* __restrict__ cdfX, const float* __restrict__ pdfX, const float4* __restrict__ data, float4* __restrict__ rec)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 c = data[i];
    rec[2 * i] = make_float4(cdfX[i], pdfX[i], c.x, c.y);
    rec[2 * i + 1] = make_float4(c.z, 0.f, 0.f, 0.f);
}

// ---- ProbeData::BuildCDF on the device (Probe.h:29-77) -----------------------------------------
// fp32 sums are not associative and the reference accumulates strictly left to right, so the
// parallelism is across rows only: one thread sums one row in order (out of LDS tiles that the
// wave loaded coalesced); a single thread then walks the row totals.  Same bits as the host helper
// fovpt_probe_build_cdf.
#define CDF_ROWS 8          // rows per block: a 2048-row probe gives 256 blocks, one per CU
#define CDF_COLS 256        // columns per tile = threads per block
#define CDF_LD (CDF_COLS + 4)   // row pitch in LDS: 16-byte reads of CDF_ROWS different rows fall into different banks
__global__ __launch_bounds__(CDF_COLS) void k_cdf_rows(int w, int h, const float4* __restrict__ data, float* __restrict__ pdfX, float* __restrict__ cdfX,
                                                      float* __restrict__ row_total)
{
    // A block = CDF_ROWS rows, walked in tiles of CDF_COLS columns.  All four waves read the tile's texels COALESCED (a wave
    // = 64 consecutive texels of one row, 1 KB) and park their luminances in LDS; lane r of wave 0 then adds up row r's
    // CDF_COLS values in order -- the fp32 sum of a row stays strictly left to right, which is what fixes its bits
    // (Probe.h:41-51) -- and all waves write weights and running sums back out, coalesced.  The next tile's texels are in
    // flight while the sums run.  (Was: one thread per row reading its row with a stride of w texels, every load a cache line
    // of its own, 32 waves on the whole chip: 1.8 ms for a 4096 x 2048 probe.)
    __shared__ __attribute__((aligned(16))) float s_w[CDF_ROWS][CDF_LD], s_c[CDF_ROWS][CDF_LD];
    const int j0 = blockIdx.x * CDF_ROWS, t = threadIdx.x;
    float run = 0.0f;                                                           // totalWeightX of row j0 + t so far (t < CDF_ROWS)
    float4 c[CDF_ROWS];
#pragma unroll
    for (int r = 0; r < CDF_ROWS; r++) c[r] = (j0 + r < h && t < w) ? data[(size_t)(j0 + r) * w + t] : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i0 = 0; i0 < w; i0 += CDF_COLS) {
#pragma unroll
        for (int r = 0; r < CDF_ROWS; r++) s_w[r][t] = c[r].x * 0.3f + c[r].y * 0.6f + c[r].z * 0.1f;      // Luminance, maths.h:165-168
        __syncthreads();
        const int in = i0 + CDF_COLS + t;
#pragma unroll
        for (int r = 0; r < CDF_ROWS; r++) c[r] = (j0 + r < h && in < w) ? data[(size_t)(j0 + r) * w + in] : make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < CDF_ROWS && j0 + t < h) {
            const int n = min(CDF_COLS, w - i0);
            int k = 0;
            for (; k + 4 <= n; k += 4) {
                const float4 v = *(const float4*)&s_w[t][k];
                float4 o;
                run += v.x; o.x = run; run += v.y; o.y = run; run += v.z; o.z = run; run += v.w; o.w = run;
                *(float4*)&s_c[t][k] = o;
            }
            for (; k < n; k++) { run += s_w[t][k]; s_c[t][k] = run; }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < CDF_ROWS; r++) {
            const int j = j0 + r, i = i0 + t;
            if (j < h && i < w) { pdfX[(size_t)j * w + i] = s_w[r][t]; cdfX[(size_t)j * w + i] = s_c[r][t]; }
        }
        __syncthreads();
    }
    if (t < CDF_ROWS && j0 + t < h) row_total[j0 + t] = run;
}
// second pass: pdf and cdf of every row times 1 / its total (the reference multiplies by the reciprocal, Probe.h:49-55)
__global__ void k_cdf_rows_scale(int w, int h, float* __restrict__ pdfX, float* __restrict__ cdfX, const float* __restrict__ row_total)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (size_t)w * h) return;
    const float invTotalWeightX = 1.0f / row_total[k / (size_t)w];
    pdfX[k] *= invTotalWeightX;
    cdfX[k] *= invTotalWeightX;
}
// (the running sum over the rows is sequential by contract -- one thread; the two divisions per row are not)
__global__ __launch_bounds__(256) void k_cdf_cols(int h, const float* __restrict__ row_total, float* __restrict__ pdfY, float* __restrict__ cdfY)
{
    // chunks of the row totals go through LDS: the block loads a chunk, thread 0 adds it up in order, the block writes the
    // running sums out.  (The one sequential thread used to read and write global memory value by value: 60 ns per row.)
    __shared__ __attribute__((aligned(16))) float s_v[2048], s_c[2048];
    __shared__ float s_total;
    if (blockIdx.x != 0) return;
    float totalWeightY = 0.0f;                                                  // thread 0's
    for (int j0 = 0; j0 < h; j0 += 2048) {
        const int n = min(2048, h - j0);
        for (int k = (int)threadIdx.x; k < n; k += (int)blockDim.x) s_v[k] = row_total[j0 + k];
        __syncthreads();
        if (threadIdx.x == 0) {
            int k = 0;
            for (; k + 4 <= n; k += 4) {
                const float4 v = *(const float4*)&s_v[k];
                float4 o;
                totalWeightY += v.x; o.x = totalWeightY; totalWeightY += v.y; o.y = totalWeightY;
                totalWeightY += v.z; o.z = totalWeightY; totalWeightY += v.w; o.w = totalWeightY;
                *(float4*)&s_c[k] = o;
            }
            for (; k < n; k++) { totalWeightY += s_v[k]; s_c[k] = totalWeightY; }
        }
        __syncthreads();
        for (int k = (int)threadIdx.x; k < n; k += (int)blockDim.x) { pdfY[j0 + k] = s_v[k]; cdfY[j0 + k] = s_c[k]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) s_total = totalWeightY;
    __syncthreads();
    const float total = s_total;
    for (int j = (int)threadIdx.x; j < h; j += (int)blockDim.x) {              // divisions here, not reciprocals (Probe.h:68-72)
        cdfY[j] /= total;
        pdfY[j] /= total;
    }
}

// ---- device self-test --------------------------------------------------------------------
__global__ void k_math(int op, const float* a, const float* b, float* out, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float r = 0.f;
    switch (op) {
    case FOVPT_OP_SIN: r = fovpt_dm_sinf(a[i]); break;
    case FOVPT_OP_COS: r = fovpt_dm_cosf(a[i]); break;
    case FOVPT_OP_ACOS: r = fovpt_dm_acosf(a[i]); break;
    case FOVPT_OP_ATAN2: r = fovpt_dm_atan2f(a[i], b[i]); break;
    case FOVPT_OP_LOG: r = fovpt_dm_logf(a[i]); break;
    case FOVPT_OP_POW: r = fovpt_dm_powf(a[i], b[i]); break;
    case FOVPT_OP_SQRT: r = sqrtf(a[i]); break;
    case FOVPT_OP_DIV: r = a[i] / b[i]; break;
    case FOVPT_OP_RSQRTD: r = rcp_of_sqrt_as_the_reference(a[i]); break;
    case FOVPT_OP_HALFPLUS: r = half_plus_as_the_reference(a[i]); break;
    case FOVPT_OP_UNORM8: r = unorm8((uint32_t)a[i] & 255u); break;
    }
    out[i] = r;
}

}  // namespace

// ------------------------------------------------------------------------------------------
int fovpt_launch_generate(hipStream_t st, const FrameDev& fd, PathState ps, RayQueue queue0, uint32_t cap, Counters* cnt, uint32_t slot_begin,
                          uint32_t slot_end, int grid, uint32_t sel)
{
    // a rank of a tile-sharded frame walks its own tiles only (one chain: a half-frame chain is a range of sample slots).
    // Its index space is padded (tiles beyond a row's end, launch indices beyond the grid's edge): a queue shard holds
    // slots / 8 + 512 entries and receives every eighth block iteration, so the space must not be larger than the slots
    // themselves -- it is not, except for grids a few launch indices wide, which go the other way.
    unsigned long long space = 0;
    for (int p = 0; p < fd.npass && p < FOVPT_MAX_PASSES; p++) {
        OwnedSpace o;
        o.init(fd, fd.pass[p]);
        space += ((unsigned long long)o.tile_rows * o.per_row * o.tile_lis * fd.pass[p].spp + FOVPT_BLOCK - 1u) / FOVPT_BLOCK * FOVPT_BLOCK;   // (64-bit: o.count may have wrapped)
    }
    const bool owned = fd.world > 1 && sel == 0u && slot_begin == 0u && slot_end == fd.total_slots && space <= (unsigned long long)fd.total_slots;
    if (owned)
        hipLaunchKernelGGL(k_generate_owned, dim3(grid), dim3(FOVPT_BLOCK), 0, st, fd, ps, queue0, cap, cnt);
    else
        hipLaunchKernelGGL(k_generate, dim3(grid), dim3(FOVPT_BLOCK), 0, st, fd, ps, queue0, cap, cnt, slot_begin, slot_end, sel);
    return owned ? 1 : 0;               // which kernel ran (fovpt_debug_generate hands it on)
}
void fovpt_launch_shade(hipStream_t st, const FrameDev& fd, SceneView sc, PathState ps, RayQueue queue_in, RayQueue queue_out,
                        ShadowQueue sq, uint32_t cap, Counters* cnt, int depth, int grid, hipEvent_t done, uint32_t sel)
{
    if (fd.options) {
        if (done) hipExtLaunchKernelGGL(k_shade<true>, dim3(grid), dim3(FOVPT_BLOCK), 0, st, nullptr, done, 0, fd, sc, ps, queue_in, queue_out, sq, cap, cnt, depth, sel);
        else hipLaunchKernelGGL(k_shade<true>, dim3(grid), dim3(FOVPT_BLOCK), 0, st, fd, sc, ps, queue_in, queue_out, sq, cap, cnt, depth, sel);
    } else {
        if (done) hipExtLaunchKernelGGL(k_shade<false>, dim3(grid), dim3(FOVPT_BLOCK), 0, st, nullptr, done, 0, fd, sc, ps, queue_in, queue_out, sq, cap, cnt, depth, sel);
        else hipLaunchKernelGGL(k_shade<false>, dim3(grid), dim3(FOVPT_BLOCK), 0, st, fd, sc, ps, queue_in, queue_out, sq, cap, cnt, depth, sel);
    }
}
void fovpt_launch_resolve(hipStream_t st, const FrameDev& fd, PathState ps, Counters* cnt, hipEvent_t done)
{
    dim3 grid((fd.w + 63) / 64, (fd.h + 3) / 4);
    if (done) hipExtLaunchKernelGGL(k_resolve, grid, dim3(FOVPT_BLOCK), 0, st, nullptr, done, 0, fd, ps, cnt);
    else hipLaunchKernelGGL(k_resolve, grid, dim3(FOVPT_BLOCK), 0, st, fd, ps, cnt);
}
void fovpt_launch_plan_owner(hipStream_t st, const FrameDev& fd, uint8_t* owner, uint32_t* block_count, uint32_t nblocks)
{
    hipLaunchKernelGGL(k_plan_owner, dim3(nblocks), dim3(FOVPT_BLOCK), 0, st, fd, owner, block_count);
}
void fovpt_launch_plan_scan_fill(hipStream_t st, uint32_t npix, uint32_t nblocks, int world, const uint8_t* owner, uint32_t* block_count,
                                 uint32_t* total, const uint32_t* rank_base, uint32_t* idx, int phase)
{
    if (phase == 0) hipLaunchKernelGGL(k_plan_scan, dim3(world), dim3(1024), 0, st, nblocks, world, block_count, total);
    else hipLaunchKernelGGL(k_plan_fill, dim3(nblocks), dim3(FOVPT_BLOCK), 0, st, npix, world, owner, block_count, rank_base, idx);
}
void fovpt_launch_gather_pack(hipStream_t st, uint32_t n, const uint32_t* idx, const uint32_t* frame, uint32_t* packed)
{
    if (n) hipLaunchKernelGGL(k_gather_pack, dim3((n + 255u) / 256u < 2048u ? (n + 255u) / 256u : 2048u), dim3(256), 0, st, n, idx, frame, packed);
}
void fovpt_launch_gather_unpack(hipStream_t st, int world, uint32_t stride, uint32_t total, const uint32_t* base, const uint32_t* idx,
                                const uint32_t* gathered, uint32_t* frame)
{
    if (total) hipLaunchKernelGGL(k_gather_unpack, dim3((total + 255u) / 256u < 2048u ? (total + 255u) / 256u : 2048u), dim3(256), 0, st, world, stride, base, idx, gathered, frame);
}
void fovpt_launch_build_guide(hipStream_t st, const float* cdf, int n, int segments, uint32_t* guide)
{
    const size_t total = (size_t)segments * (n + 2);
    hipLaunchKernelGGL(k_build_guide, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, cdf, n, segments, guide);
}
void fovpt_launch_probe_records(hipStream_t st, size_t n, const float* cdfX, const float* pdfX, const float4* data, float4* rec)
{
    hipLaunchKernelGGL(k_probe_records, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, cdfX, pdfX, data, rec);
}
void fovpt_launch_build_cdf(hipStream_t st, int w, int h, const float4* data, float* pdfX, float* cdfX, float* pdfY, float* cdfY, float* row_total)
{
    hipLaunchKernelGGL(k_cdf_rows, dim3((h + CDF_ROWS - 1) / CDF_ROWS), dim3(CDF_COLS), 0, st, w, h, data, pdfX, cdfX, row_total);
    hipLaunchKernelGGL(k_cdf_rows_scale, dim3((unsigned)(((size_t)w * h + 255) / 256)), dim3(256), 0, st, w, h, pdfX, cdfX, row_total);
    hipLaunchKernelGGL(k_cdf_cols, dim3(1), dim3(256), 0, st, h, row_total, pdfY, cdfY);
}
void fovpt_launch_math(hipStream_t st, int op, const float* a, const float* b, float* out, size_t n)
{
    hipLaunchKernelGGL(k_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, op, a, b, out, n);
}
