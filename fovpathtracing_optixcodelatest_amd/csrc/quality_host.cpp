// quality_host.cpp -- fovpt_quality on host images and the scores of a record: fovpt_quality_host, fovpt_quality_mse / _psnr /
// _ssim / _score (include/fovpt.h; the definition, operation by operation: tests/quality_ref.py).  Host-only
// C++ without a context or a device: compiled into libfovpt.so and into libfovpt_loader.so, the library for machines without ROCm.
// The pixel classes, which the device takes from the rendered frame's writer search, are handed in.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../include/fovpt.h"

void fovpt_internal_set_error(const char* text);      // fovpt_api.hip / loader_host.cpp: the text fovpt_last_error(NULL) returns

namespace {

int refuse(const char* why)
{
    char buf[160];
    snprintf(buf, sizeof(buf), "fovpt_quality_host: %s", why);
    fovpt_internal_set_error(buf);
    return FOVPT_E_INVALID;
}

inline int64_t luma(uint32_t p) { return (int64_t)((54u * (p & 255u) + 183u * ((p >> 8) & 255u) + 19u * ((p >> 16) & 255u) + 128u) >> 8); }

// the floor square root of d (Newton's iteration on integers from above: exact, no floating point)
uint64_t isqrt(uint64_t d)
{
    if (d < 2) return d;
    uint64_t r = (uint64_t)1 << 32;                    // (>= sqrt(d) for every 64-bit d)
    for (;;) {
        const uint64_t n = (r + d / r) >> 1;
        if (n >= r) return r;
        r = n;
    }
}

// a pixel's ring.  |dx| or |dy| >= 2^22 is ring 63 without the square (isqrt(d2) >= 2^22 > 63 * FOVPT_QUALITY_MAX_RING_WIDTH), so d2
// never leaves 64 bits whatever the gaze
uint32_t ring_of(int64_t dx, int64_t dy, int64_t ring_width)
{
    const uint64_t ax = (uint64_t)(dx < 0 ? -dx : dx), ay = (uint64_t)(dy < 0 ? -dy : dy);
    if (ax >= (1ull << 22) || ay >= (1ull << 22)) return FOVPT_QUALITY_RINGS - 1;
    const uint64_t ring = isqrt(ax * ax + ay * ay) / (uint64_t)ring_width;
    return (uint32_t)(ring < FOVPT_QUALITY_RINGS - 1 ? ring : FOVPT_QUALITY_RINGS - 1);
}

double nan_() { return std::numeric_limits<double>::quiet_NaN(); }

// the classes cls stands for (-1: all but UNWRITTEN); false: none
bool class_range(int cls, int& k0, int& k1)
{
    if (cls == -1) { k0 = 0; k1 = FOVPT_QUALITY_UNWRITTEN; return true; }
    if (cls < 0 || cls >= FOVPT_QUALITY_CLASSES) return false;
    k0 = cls; k1 = cls + 1;
    return true;
}

}  // namespace

int fovpt_quality_host(const uint32_t* test, const uint32_t* ref, int w, int h, const uint8_t* classes, int64_t gaze_x, int64_t gaze_y,
                       const fovpt_quality_config* qc, fovpt_quality_sums* out)
{
    if (!test || !ref || !qc || !out) return refuse("null argument");
    if (w < 1 || h < 1 || (uint64_t)w * (uint64_t)h >= (1ull << 31)) return refuse("width or height below 1, or 2^31 pixels or more");
    if (qc->flags & ~(FOVPT_QUALITY_SSIM | FOVPT_QUALITY_PROFILE)) return refuse("unknown flag bits");
    if (qc->ring_width < 1 || qc->ring_width > FOVPT_QUALITY_MAX_RING_WIDTH) return refuse("ring_width outside 1 .. 65536");
    for (int32_t r : qc->_reserved)
        if (r != 0) return refuse("reserved fields must be 0");
    const size_t npix = (size_t)w * (size_t)h;
    if (classes)
        for (size_t i = 0; i < npix; i++)
            if (classes[i] >= FOVPT_QUALITY_CLASSES) return refuse("a class byte outside 0 .. 4");
    fovpt_quality_sums s;
    memset(&s, 0, sizeof(s));
    s.width = (uint32_t)w; s.height = (uint32_t)h; s.ring_width = (uint32_t)qc->ring_width; s.flags = (uint32_t)qc->flags;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * (size_t)w + (size_t)x;
            const uint32_t t = test[i], f = ref[i];
            const int k = classes ? classes[i] : FOVPT_QUALITY_UNIFORM;
            uint64_t sq = 0;
            uint32_t mx = 0;
            for (int c = 0; c < 3; c++) {
                const int32_t d = (int32_t)((t >> (8 * c)) & 255u) - (int32_t)((f >> (8 * c)) & 255u);
                const uint32_t a = (uint32_t)(d < 0 ? -d : d);
                s.sq_err[k][c] += (uint64_t)(a * a);
                sq += (uint64_t)(a * a);
                mx = a > mx ? a : mx;
            }
            s.pixels[k] += 1;
            s.differing[k] += mx != 0u;
            s.max_err[k] = mx > s.max_err[k] ? mx : s.max_err[k];
            if (qc->flags & FOVPT_QUALITY_PROFILE) {
                const uint32_t ring = ring_of((int64_t)x - gaze_x, (int64_t)y - gaze_y, qc->ring_width);
                s.ring_pixels[ring] += 1;
                s.ring_sq_err[ring] += sq;
            }
        }
    if (qc->flags & FOVPT_QUALITY_SSIM)
        for (int y0 = 0; y0 + 8 <= h; y0 += 4)
            for (int x0 = 0; x0 + 8 <= w; x0 += 4) {
                int64_t sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
                for (int v = 0; v < 8; v++)
                    for (int u = 0; u < 8; u++) {
                        const size_t i = (size_t)(y0 + v) * (size_t)w + (size_t)(x0 + u);
                        const int64_t a = luma(test[i]), b = luma(ref[i]);
                        sx += a; sy += b; sxx += a * a; syy += b * b; sxy += a * b;
                    }
                const int64_t C1 = 26634, C2 = 239708;
                const int64_t A = 2 * sx * sy + C1, B = 2 * (64 * sxy - sx * sy) + C2, C = sx * sx + sy * sy + C1,
                              D = (64 * sxx - sx * sx) + (64 * syy - sy * sy) + C2;
                const int64_t N = A * B, M = C * D;                   // (|N|, M < 2^57; M > 0)
                const double quot = (double)N / (double)M;
                const int64_t q = (int64_t)std::rint(quot * 1048576.0);
                const size_t ic = (size_t)(y0 + 4) * (size_t)w + (size_t)(x0 + 4);
                const int k = classes ? classes[ic] : FOVPT_QUALITY_UNIFORM;
                s.windows[k] += 1;
                s.ssim_q20[k] += q;
            }
    *out = s;
    return FOVPT_OK;
}

double fovpt_quality_mse(const fovpt_quality_sums* s, int cls)
{
    int k0, k1;
    if (!s || !class_range(cls, k0, k1)) return nan_();
    uint64_t sq = 0, n = 0;
    for (int k = k0; k < k1; k++) { sq += (s->sq_err[k][0] + s->sq_err[k][1]) + s->sq_err[k][2]; n += s->pixels[k]; }
    if (n == 0) return nan_();
    return (double)sq / (3.0 * (double)n);
}

double fovpt_quality_psnr(const fovpt_quality_sums* s, int cls)
{
    const double mse = fovpt_quality_mse(s, cls);
    if (mse != mse) return mse;
    if (mse == 0.0) return std::numeric_limits<double>::infinity();
    return 10.0 * std::log10(65025.0 / mse);
}

double fovpt_quality_ssim(const fovpt_quality_sums* s, int cls)
{
    int k0, k1;
    if (!s || !class_range(cls, k0, k1)) return nan_();
    int64_t q = 0;
    uint64_t n = 0;
    for (int k = k0; k < k1; k++) { q += s->ssim_q20[k]; n += s->windows[k]; }
    if (n == 0) return nan_();
    return (double)q / (1048576.0 * (double)n);
}

double fovpt_quality_score(const fovpt_quality_sums* s, const double weights[FOVPT_QUALITY_CLASSES])
{
    if (!s || !weights) return nan_();
    double num = 0.0, den = 0.0;
    for (int k = 0; k < FOVPT_QUALITY_CLASSES; k++) {
        const uint64_t sq = (s->sq_err[k][0] + s->sq_err[k][1]) + s->sq_err[k][2];
        num += weights[k] * (double)sq;
        den += weights[k] * (double)s->pixels[k];
    }
    if (!(den > 0.0)) return nan_();
    return num / (3.0 * den);
}
