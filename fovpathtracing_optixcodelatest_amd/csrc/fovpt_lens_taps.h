// fovpt_lens_taps.h -- fovpt_lens: from a source position (fx, fy) in pixels to validity and tap indices (steps 7 and 8's index part
// of the definition in include/fovpt.h), in one place for k_lens (lens.hip) and for a CPU program (tests/cpp/lens_taps_test.cpp),
// which sweeps it under the host sanitizers.  Compiles for host and device alike; nothing here reads memory.
//
// A tap coordinate is kept as a WRAPPING uint32: inside the accepted range floor(f) lies in [-2, n + 2] with n < 2^31, so a
// coordinate left of the frame becomes a value of 2^32 - 3 or more and one right of it stays below 2^31 + 4: neither is ever
// below n, and `c < n` in unsigned is the whole inside test.  No float outside [0, 2^32) is ever converted to an integer.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FOVPT_LENS_HD __host__ __device__
#else
#define FOVPT_LENS_HD
#endif

#define FOVPT_LENS_TAPS_NEAREST 0       // FOVPT_LENS_* of include/fovpt.h (this header stands alone)
#define FOVPT_LENS_TAPS_BILINEAR 1
#define FOVPT_LENS_TAPS_BICUBIC 2

// One axis of a window: its first tap and the fraction t of the filter (NEAREST: unused, 0)
struct LensAxis {
    uint32_t first;
    float t;
};

// the taps of a window along one axis: 1, 2 or 4
FOVPT_LENS_HD inline int lens_tap_count(int filter) { return filter == FOVPT_LENS_TAPS_NEAREST ? 1 : filter == FOVPT_LENS_TAPS_BILINEAR ? 2 : 4; }

// Step 7's range test and step 8's first tap along an axis of n pixels.  false: the channel is invalid (NaN fails the test).
FOVPT_LENS_HD inline bool lens_axis(float f, int32_t n, int filter, LensAxis& a)
{
    a.first = 0u; a.t = 0.0f;
    if (!(f >= -2.0f && f <= (float)n + 1.0f)) return false;
    const bool nearest = filter == FOVPT_LENS_TAPS_NEAREST;
    const float fl = floorf(nearest ? f + 0.5f : f);                       // in [-2, n + 2]: |fl| < 2^32
    if (!nearest) a.t = f - fl;
    const uint32_t u = fl < 0.0f ? 0u - (uint32_t)(-fl) : (uint32_t)fl;
    a.first = filter == FOVPT_LENS_TAPS_BICUBIC ? u - 1u : u;
    return true;
}

// tap i (0 .. lens_tap_count - 1) of an axis, and whether it lies inside the frame (outside: the tap reads the border)
FOVPT_LENS_HD inline uint32_t lens_tap(const LensAxis& a, int i) { return a.first + (uint32_t)i; }
FOVPT_LENS_HD inline bool lens_tap_inside(uint32_t c, int32_t n) { return c < (uint32_t)n; }

// Both axes: false where the channel is invalid, and then no tap is read
FOVPT_LENS_HD inline bool lens_taps(float fx, float fy, int32_t w, int32_t h, int filter, LensAxis& ax, LensAxis& ay)
{
    const bool okx = lens_axis(fx, w, filter, ax), oky = lens_axis(fy, h, filter, ay);
    return okx && oky;
}
