// The index function of fovpt_lens (csrc/fovpt_lens_taps.h: from a source position to validity and tap indices) on the host, under
// the address and undefined-behaviour sanitizers (float -> integer conversions included): a stand-alone program, no library.
//
// Per axis -- the function is separable -- and per filter, for the frame extents 1, 2, 3, 17, 33, 109 and 193:
//   NaN, +-inf, +-0, +-2^31, +-3e38, the smallest denormals and normals, FLT_MAX,
//   every float within +-4 of the edge n where n - 4 >= 4 (half a million floats an extent);
//   around the edge 0, where +-4 holds 2^31 floats: every float within 2^-10 of a multiple of 1/2 in [-4, 4] -- where floor, the
//   NEAREST rounding and the range test can turn --, every 61st float in between down to 1/4, and below 1/4 the 4096 floats at
//   either end of every binade and of the denormals (between them the function takes one path: floor 0 or -1).
// Every result is compared with an independent evaluation in binary64 and 64-bit integers, and every tap must be flagged outside
// the frame or lie inside it.  Then both axes together over the cross product of the special values, indexing a guarded frame.
#include <cmath>
#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fovpt_lens_taps.h"

static unsigned long long checked = 0, valid_seen = 0, border_seen = 0, inside_seen = 0;

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t to_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// the definition, independently: binary64 and int64
static bool expect_axis(float f, int n, int filter, long long& first, float& t)
{
    if (!(f >= -2.0f && f <= (float)n + 1.0f)) return false;
    const float g = filter == FOVPT_LENS_TAPS_NEAREST ? f + 0.5f : f;      // (one binary32 sum, as the definition has it)
    const double fl = std::floor((double)g);
    first = (long long)fl - (filter == FOVPT_LENS_TAPS_BICUBIC ? 1 : 0);
    t = filter == FOVPT_LENS_TAPS_NEAREST ? 0.0f : f - (float)fl;
    return true;
}

static int check_axis(float f, int n, int filter)
{
    LensAxis a;
    long long first = 0;
    float t = 0.0f;
    const bool ok = lens_axis(f, n, filter, a), want = expect_axis(f, n, filter, first, t);
    checked++;
    if (ok != want) { printf("validity of %a (n %d, filter %d): %d, expected %d\n", f, n, filter, (int)ok, (int)want); return 1; }
    if (!ok) return 0;
    valid_seen++;
    if (to_bits(a.t) != to_bits(t)) { printf("t of %a (n %d, filter %d): %a, expected %a\n", f, n, filter, a.t, t); return 1; }
    if (filter != FOVPT_LENS_TAPS_NEAREST && !(a.t >= 0.0f && a.t <= 1.0f)) { printf("t of %a outside [0, 1]: %a\n", f, a.t); return 1; }
    const int taps = lens_tap_count(filter);
    for (int i = 0; i < taps; i++) {
        const uint32_t c = lens_tap(a, i);
        const long long e = first + i;
        const bool in = lens_tap_inside(c, n), want_in = e >= 0 && e < n;
        if (in != want_in || (in && (long long)c != e)) {
            printf("tap %d of %a (n %d, filter %d): %u %s, expected %lld %s\n", i, f, n, filter, c, in ? "inside" : "border", e, want_in ? "inside" : "border");
            return 1;
        }
        if (in) inside_seen++; else border_seen++;
    }
    return 0;
}

// every float from lo to hi (same sign, |lo| <= |hi| in bits order)
static int sweep_bits(uint32_t lo, uint32_t hi, int n, int filter, uint32_t step = 1u)
{
    for (uint32_t u = lo; u <= hi; u += step)                             // (hi is far below 2^32 - step)
        if (check_axis(from_bits(u), n, filter)) return 1;
    return check_axis(from_bits(hi), n, filter);
}

static int sweep_range(float lo, float hi, int n, int filter, uint32_t step = 1u)   // the floats of [lo, hi], lo and hi of one sign, neither 0
{
    if (lo >= 0.0f) return sweep_bits(to_bits(lo), to_bits(hi), n, filter, step);
    return sweep_bits(to_bits(hi), to_bits(lo), n, filter, step);          // (negative floats: the bits grow with the magnitude)
}

int main()
{
    const int extents[] = {1, 2, 3, 17, 33, 109, 193};
    const float tiny = 0.25f;
    const float special[] = {NAN, -NAN, INFINITY, -INFINITY, 0.0f, -0.0f, 2147483648.0f, -2147483648.0f, 3e38f, -3e38f, FLT_MAX, -FLT_MAX,
                             FLT_MIN, -FLT_MIN, from_bits(1u), from_bits(0x80000001u), 4294967296.0f, -4294967296.0f, 2147483520.0f, 16777216.0f,
                             -0.5f, 0.5f, -1.0f, -2.0f, from_bits(0xc0000001u) /* below -2 */, from_bits(0xbfffffffu) /* above -2 */};
    for (int filter = 0; filter < 3; filter++) {
        for (int n : extents) {
            for (float f : special)
                if (check_axis(f, n, filter)) return 1;
            // around the edge 0: [-4, -1/4] and [1/4, 4], and the ends of every binade below
            if (sweep_range(-4.0f, -tiny, n, filter, 61u) || sweep_range(tiny, 4.0f, n, filter, 61u)) return 1;
            for (int m = -8; m <= 8; m++) {                                // the multiples of 1/2: where floor, the rounding and the range test turn
                if (m == 0) continue;                                      // (0: the binade ends below)
                const float c = 0.5f * (float)m, d = 0.0009765625f;
                if (sweep_range(c - d, c + d, n, filter)) return 1;
            }
            for (uint32_t sign = 0; sign < 2; sign++)
                for (uint32_t e = 0; e <= 125; e++) {                      // exponent fields of the denormals .. 1/4
                    const uint32_t base = (sign << 31) | (e << 23);
                    if (sweep_bits(base, base + 4095u, n, filter) || sweep_bits(base + 0x7ff000u, base + 0x7fffffu, n, filter)) return 1;
                }
            // around the edge n (where that is not the sweep above again)
            const float lo = (float)n - 4.0f, hi = (float)n + 4.0f;
            if (sweep_range(lo > 4.0f ? lo : 4.0f, hi, n, filter)) return 1;
        }
        // extents at which float -> integer conversion is closest to its limits
        const int large[] = {16777217, 1073741824, 2147483647};
        for (int n : large) {
            for (float f : special)
                if (check_axis(f, n, filter)) return 1;
            const float e = (float)n;
            if (sweep_bits(to_bits(e) - 4096u, to_bits(e) + 4096u, n, filter)) return 1;
        }
    }

    // both axes: a frame of w x h pixels between guard zones, indexed through the taps
    const int sizes[][2] = {{1, 1}, {2, 1}, {1, 3}, {33, 17}, {193, 109}};
    for (const auto& s : sizes) {
        const int w = s[0], h = s[1];
        std::vector<float> xs(special, special + sizeof(special) / sizeof(special[0])), ys = xs;
        for (int k = -5 * 8; k <= 5 * 8; k++) {
            xs.push_back(k * 0.125f); xs.push_back((float)w + k * 0.125f);
            ys.push_back(k * 0.125f); ys.push_back((float)h + k * 0.125f);
        }
        std::vector<unsigned char> frame((size_t)w * h, 1);                // ASan guards what lies around it
        for (int filter = 0; filter < 3; filter++)
            for (float fy : ys)
                for (float fx : xs) {
                    LensAxis ax, ay;
                    long long ex = 0, ey = 0;
                    float tx, ty;
                    const bool want = expect_axis(fx, w, filter, ex, tx) & expect_axis(fy, h, filter, ey, ty);
                    if (lens_taps(fx, fy, w, h, filter, ax, ay) != want) { printf("validity of (%a, %a) in %d x %d\n", fx, fy, w, h); return 1; }
                    checked++;
                    if (!want) continue;
                    for (int j = 0; j < lens_tap_count(filter); j++)
                        for (int i = 0; i < lens_tap_count(filter); i++) {
                            const uint32_t qx = lens_tap(ax, i), qy = lens_tap(ay, j);
                            if (!lens_tap_inside(qx, w) || !lens_tap_inside(qy, h)) continue;
                            const uint32_t q = qy * (uint32_t)w + qx;      // as the kernel forms it
                            if (frame[q] != 1) { printf("tap (%u, %u) reads outside the frame\n", qx, qy); return 1; }
                        }
                }
    }
    if (!valid_seen || !border_seen || !inside_seen) { printf("the sweep is vacuous\n"); return 1; }
    printf("ok: %llu positions, %llu valid, %llu taps inside, %llu border\n", checked, valid_seen, inside_seen, border_seen);
    return 0;
}
