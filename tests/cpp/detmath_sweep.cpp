// Host-only sweep of include/fovpt_detmath.h over whole production domains, against the C library's binary64 functions
// (independent of tests/detmath_ref.py, which uses numpy):
//
//     sin, cos        every float in [0, 2*pi]
//     acos            every float in [-1, 1]
//     log             every positive finite float
//     pow(x, 1/2.4f)  every float in (0, 1]
//
//   g++ -O2 -std=c++14 -ffp-contract=off -pthread -I include tests/cpp/detmath_sweep.cpp -o detmath_sweep
//   ./detmath_sweep            every float (about a minute on 16 threads)
//   ./detmath_sweep 64         every 64th float (what tests/test_detmath_cpu.py runs)
//
// Prints, per function, the largest error in binary32 ulps of the binary64 value and where it occurs, and a digest of all sin and
// cos result bits in argument order (FNV-1a per block of 2^20 arguments, folded in block order: the thread count does not enter).
// The binary64 library is itself good to about an ulp of binary64 = 2^-29 binary32 ulp, which bounds what the maxima can mean.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "fovpt_detmath.h"

namespace {

const int kThreads = 16;
const uint64_t kBlock = 1u << 20;              // arguments per work item

float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
uint32_t to_bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// |got - want| in binary32 ulps of `want` (finite); a zero is matched by a zero only
double ulp_error(float got, double want)
{
    if (want == 0.0) return got == 0.0f ? 0.0 : INFINITY;
    if (!(std::fabs((double)got) <= 3.5e38)) return INFINITY;
    const int e = std::max(std::ilogb(want), -126) - 23;
    return std::fabs((double)got - want) / std::ldexp(1.0, e);
}

struct Worst { double err = 0.0; uint32_t at = 0; void see(double e, uint32_t b) { if (e > err) { err = e; at = b; } } };

uint64_t fnv(uint64_t h, uint32_t v)
{
    for (int k = 0; k < 4; k++) { h ^= (v >> (8 * k)) & 0xffu; h *= 0x100000001b3ull; }
    return h;
}

enum Fn { SINCOS, ACOS, LOG, POW };

// arguments: bit patterns first, first + stride, ... <= last, with `sign` or'ed in
struct Range { Fn fn; uint32_t first, last, sign; };

struct Result { Worst w[2]; std::vector<uint64_t> block_hash; };

void run(const Range& r, uint32_t stride, Result& res)
{
    const uint64_t count = ((uint64_t)r.last - r.first) / stride + 1;
    const uint64_t blocks = (count + kBlock - 1) / kBlock;
    res.block_hash.assign(blocks, 0);
    std::atomic<uint64_t> next(0);
    std::vector<Worst> tw(kThreads * 2);
    std::vector<std::thread> th;
    const float inv_gamma = 1.0f / 2.4f;
    for (int t = 0; t < kThreads; t++)
        th.emplace_back([&, t]() {
            Worst w0, w1;
            for (;;) {
                const uint64_t b = next.fetch_add(1);
                if (b >= blocks) break;
                uint64_t h = 0xcbf29ce484222325ull;
                const uint64_t i1 = std::min(count, (b + 1) * kBlock);
                for (uint64_t i = b * kBlock; i < i1; i++) {
                    const uint32_t bits = (uint32_t)(r.first + i * stride) | r.sign;
                    const float x = from_bits(bits);
                    switch (r.fn) {
                    case SINCOS: {
                        float s, c;
                        fovpt_dm_sincos(x, &s, &c);
                        w0.see(ulp_error(s, std::sin((double)x)), bits);
                        w1.see(ulp_error(c, std::cos((double)x)), bits);
                        h = fnv(fnv(h, to_bits(s)), to_bits(c));
                        break;
                    }
                    case ACOS: w0.see(ulp_error(fovpt_dm_acosf(x), std::acos((double)x)), bits); break;
                    case LOG: w0.see(ulp_error(fovpt_dm_logf(x), std::log((double)x)), bits); break;
                    case POW: w0.see(ulp_error(fovpt_dm_powf(x, inv_gamma), std::pow((double)x, (double)inv_gamma)), bits); break;
                    }
                }
                res.block_hash[b] = h;
            }
            tw[2 * t] = w0;
            tw[2 * t + 1] = w1;
        });
    for (auto& t : th) t.join();
    for (int t = 0; t < kThreads; t++) {
        // ties between threads resolved by the lower argument, so the report does not depend on scheduling
        for (int k = 0; k < 2; k++) {
            const Worst& w = tw[2 * t + k];
            if (w.err > res.w[k].err || (w.err == res.w[k].err && w.err > 0 && w.at < res.w[k].at)) res.w[k] = w;
        }
    }
}

void report(const char* name, const Worst& w)
{
    std::printf("%s max_ulp=%.9f at=0x%08x (%.9g)\n", name, w.err, w.at, (double)from_bits(w.at));
}

}  // namespace

int main(int argc, char** argv)
{
    const long s = argc > 1 ? std::atol(argv[1]) : 1;
    if (s < 1 || s > (1 << 20)) { std::fprintf(stderr, "usage: %s [stride 1..2^20]\n", argv[0]); return 2; }
    const uint32_t stride = (uint32_t)s;
    const uint32_t two_pi = to_bits(3.141592653589793f * 2.0f), one = to_bits(1.0f), flt_max = 0x7f7fffffu;
    std::printf("stride=%u threads=%d\n", stride, kThreads);

    Result sc;
    run(Range{SINCOS, 0u, two_pi, 0u}, stride, sc);
    report("sin", sc.w[0]);
    report("cos", sc.w[1]);
    uint64_t d = 0xcbf29ce484222325ull;
    for (uint64_t h : sc.block_hash) { d = fnv(d, (uint32_t)h); d = fnv(d, (uint32_t)(h >> 32)); }
    std::printf("sincos_digest=%016llx\n", (unsigned long long)d);

    Result ap, an;
    run(Range{ACOS, 0u, one, 0u}, stride, ap);
    run(Range{ACOS, 0u, one, 0x80000000u}, stride, an);
    report("acos", an.w[0].err > ap.w[0].err ? an.w[0] : ap.w[0]);

    Result lg;
    run(Range{LOG, 1u, flt_max, 0u}, stride, lg);
    report("log", lg.w[0]);

    Result pw;
    run(Range{POW, 1u, one, 0u}, stride, pw);
    report("pow", pw.w[0]);
    return 0;
}
