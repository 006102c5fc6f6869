// tools/micro/l2_stream.hip -- can a load or store flavour keep a once-touched stream from evicting a re-read table out of L2?
//
// The frame's situation in small: every wave walks a TABLE by random 128-byte lines, one quad per line and two 16-byte loads per
// lane as k_traverse fetches a node (a dependent chain through a permutation, as in gather_rate.hip), and beside every two steps
// it reads SP x 1 KB of a STREAM that the launch before wrote and writes SP x 1 KB for the launch after: SP = 3 is 1.5 stream
// bytes per gathered byte, the frame's ratio of stream misses to scene misses (EXPERIMENTS.md, "After round 4").  The table is
// read by every XCD, so each XCD's 4 MiB L2 would have to hold all of it: 2 MB fits, 4 MB is the edge, 8 and 16 MB do not.  The
// stream wraps in 64 MB per buffer (far beyond L2, inside the Infinity Cache, as the frame's queues are).
//   flavours of the stream: loads plain / nt / sc1, stores plain / nt / sc1 (the 16-byte sc1 store is fovpt_stream.h's)
//   output: ns per gather step and wave for every table size and flavour; "none" = the table alone
// Second table: a wave's 16-byte loads with FOUR lanes per address (a quad fetching its ray record) against one lane per
// address, plain and nt, over 64 MB: what the L1 bypass costs when a quad shares a record.
//
//   hipcc -O3 --offload-arch=gfx950 tools/micro/l2_stream.hip -o tools/micro/l2_stream && tools/micro/l2_stream [SP]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include <utility>

typedef float F4 __attribute__((ext_vector_type(4)));
typedef uint32_t U4 __attribute__((ext_vector_type(4)));
enum { PLAIN = 0, NT = 1, SC1 = 2 };

// aux 16 = sc1 on gfx950; the load is one the compiler counts in its waits
__device__ inline __amdgpu_buffer_rsrc_t rsrc_of(const void* base, uint32_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
template <int LD>
__device__ inline F4 ld16(const F4* base, uint32_t idx, uint32_t bytes)
{
    if (LD == PLAIN) return base[idx];
    if (LD == NT) return __builtin_nontemporal_load(base + idx);
    const U4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc_of(base, bytes), idx << 4, 0, 16);
    F4 r;
    r.x = __uint_as_float(v.x); r.y = __uint_as_float(v.y); r.z = __uint_as_float(v.z); r.w = __uint_as_float(v.w);
    return r;
}
template <int ST>
__device__ inline void st16(F4* p, F4 v)
{
    if (ST == PLAIN) *p = v;
    else if (ST == NT) __builtin_nontemporal_store(v, p);
    else asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
}

// grid x 256 threads; pairs: iterations of two gather steps; sp: stream kilobytes read and written per wave and pair
template <int LD, int ST>
__global__ __launch_bounds__(256, 8) void k_mix(const float4* __restrict__ tab, uint32_t mask, int pairs, int sp, const F4* __restrict__ rd, F4* __restrict__ wr,
                                                uint32_t smask, float4* __restrict__ out)
{
    const uint32_t j = threadIdx.x & 3u, lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t node = ((blockIdx.x * 64u + (threadIdx.x >> 2)) * 2654435761u) & mask;
    float acc = 0.f;
    F4 sv;
    sv.x = (float)lane; sv.y = 1.f; sv.z = 2.f; sv.w = 3.f;
    for (int i = 0; i < pairs; i++) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const float4* p = (const float4*)((const char*)tab + (((size_t)node << 7) | (j << 5)));
            const float4 a = p[0], b = p[1];
            acc += (a.x + a.y) + (a.w + b.x) + (b.y + b.z) + b.w;
            node = __float_as_uint(a.z) & mask;
        }
        const uint32_t s0 = ((wave * (uint32_t)pairs + (uint32_t)i) * (uint32_t)sp) * 64u + lane;
        for (int k = 0; k < sp; k++) {
            const uint32_t idx = (s0 + (uint32_t)k * 64u) & smask;
            const F4 v = ld16<LD>(rd, idx, (smask + 1u) << 4);
            acc += (v.x + v.y) + (v.z + v.w);
            st16<ST>(wr + idx, sv);
        }
    }
    out[blockIdx.x * 256 + threadIdx.x] = make_float4(acc, (float)node, 0, 0);
}

// a wave's 16-byte loads over a large buffer: SHARE lanes per address
template <int LD, int SHARE>
__global__ __launch_bounds__(256, 8) void k_share(const F4* __restrict__ buf, uint32_t smask, int iters, float4* __restrict__ out)
{
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t per = 64u / SHARE;
    float acc = 0.f;
    for (int i = 0; i < iters; i++) {
        const uint32_t idx = ((wave * (uint32_t)iters + (uint32_t)i) * per + lane / SHARE) & smask;
        const F4 v = ld16<LD>(buf, idx, (smask + 1u) << 4);
        acc += (v.x + v.y) + (v.z + v.w);
    }
    out[blockIdx.x * 256 + threadIdx.x] = make_float4(acc, 0, 0, 0);
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

typedef void (*MixFn)(const float4*, uint32_t, int, int, const F4*, F4*, uint32_t, float4*);
typedef void (*ShareFn)(const F4*, uint32_t, int, float4*);

int main(int argc, char** argv)
{
    const int sp = argc > 1 ? atoi(argv[1]) : 3;
    if (sp < 0 || sp > 16) { fprintf(stderr, "SP in 0..16\n"); return 2; }
    hipDeviceProp_t pr;
    CK(hipGetDeviceProperties(&pr, 0));
    const int cus = pr.multiProcessorCount, grid = cus * 8, pairs = 100;      // 8 waves per SIMD
    const size_t sbytes = (size_t)64 << 20;
    const uint32_t smask = (uint32_t)(sbytes / 16 - 1);
    F4 *s0, *s1;
    float4* out;
    CK(hipMalloc(&s0, sbytes)); CK(hipMalloc(&s1, sbytes)); CK(hipMalloc(&out, sizeof(float4) * 256 * (size_t)grid));
    CK(hipMemset(s0, 0, sbytes)); CK(hipMemset(s1, 0, sbytes));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    struct Case { const char* name; MixFn fn; bool stream; };
    const Case cases[] = {
        {"none (table alone)", k_mix<PLAIN, PLAIN>, false},
        {"ld plain, st plain", k_mix<PLAIN, PLAIN>, true},
        {"ld nt,    st nt   ", k_mix<NT, NT>, true},
        {"ld plain, st nt   ", k_mix<PLAIN, NT>, true},
        {"ld plain, st sc1  ", k_mix<PLAIN, SC1>, true},
        {"ld nt,    st plain", k_mix<NT, PLAIN>, true},
        {"ld sc1,   st plain", k_mix<SC1, PLAIN>, true},
        {"ld nt,    st sc1  ", k_mix<NT, SC1>, true},
        {"ld sc1,   st sc1  ", k_mix<SC1, SC1>, true},
    };
    printf("l2_stream: %d CUs, grid %d x 256, %d pairs of gather steps, stream %d KB read + %d KB written per wave and pair (%.2f stream bytes per gathered byte)\n",
           cus, grid, pairs, sp, sp, sp * 2048.0 / 4096.0);
    for (size_t mb : {2, 4, 8, 16}) {
        const size_t bytes = mb << 20, nrec = bytes / 128;
        std::vector<uint32_t> h(bytes / 4, 0x3f800000u), perm(nrec);
        for (size_t r = 0; r < nrec; r++) perm[r] = (uint32_t)r;
        uint32_t s = 777;
        for (size_t r = nrec - 1; r > 0; r--) { s = s * 1664525u + 1013904223u; const size_t o = (size_t)(((uint64_t)(s >> 4) * (r + 1)) >> 28); std::swap(perm[r], perm[o]); }
        for (size_t r = 0; r < nrec; r++)
            for (size_t jj = 0; jj < 4; jj++) h[(r * 128 + jj * 32) / 4 + 2] = perm[r];
        float4* tab;
        CK(hipMalloc(&tab, bytes)); CK(hipMemcpy(tab, h.data(), bytes, hipMemcpyHostToDevice));
        for (const Case& c : cases) {
            const int spc = c.stream ? sp : 0;
            float best = 1e30f;
            // launch n reads what launch n - 1 wrote; the first is the warm-up
            for (int rep = 0; rep < 4; rep++) {
                CK(hipEventRecord(e0));
                hipLaunchKernelGGL(c.fn, dim3(grid), dim3(256), 0, 0, tab, (uint32_t)(nrec - 1), pairs, spc, rep & 1 ? s1 : s0, rep & 1 ? s0 : s1, smask, out);
                CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
                float ms;
                CK(hipEventElapsedTime(&ms, e0, e1));
                if (rep > 0 && ms < best) best = ms;
            }
            printf("table %2zu MB  %s  %7.1f us per launch  %6.0f ns per gather step and wave\n", mb, c.name, best * 1e3, best * 1e6 / (2.0 * pairs));
        }
        CK(hipFree(tab));
    }
    struct SCase { const char* name; ShareFn fn; int share; };
    const SCase scases[] = {
        {"1 lane  per address, plain", k_share<PLAIN, 1>, 1}, {"1 lane  per address, nt   ", k_share<NT, 1>, 1}, {"1 lane  per address, sc1  ", k_share<SC1, 1>, 1},
        {"4 lanes per address, plain", k_share<PLAIN, 4>, 4}, {"4 lanes per address, nt   ", k_share<NT, 4>, 4}, {"4 lanes per address, sc1  ", k_share<SC1, 4>, 4},
    };
    const int iters = 200;
    for (const SCase& c : scases) {
        float best = 1e30f;
        for (int rep = 0; rep < 4; rep++) {
            CK(hipEventRecord(e0));
            hipLaunchKernelGGL(c.fn, dim3(grid), dim3(256), 0, 0, s0, smask, iters, out);
            CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (rep > 0 && ms < best) best = ms;
        }
        const double loads = (double)grid * 4 * iters;
        printf("16-byte loads, %s  %7.1f us  %6.2f ns per wave load at 8 waves per SIMD  %6.0f GB/s of distinct bytes\n", c.name, best * 1e3, best * 1e6 / iters,
               loads * (64 / c.share) * 16 / (best * 1e6));
    }
    CK(hipDeviceSynchronize());
    return 0;
}
