/*
 * fovpt_detmath.h -- deterministic transcendental functions (part of libfovpt's contract).
 *
 * The reference calls sinf/cosf/acosf/atan2f/logf/powf from the CUDA math library
 * (built with --use_fast_math, CMakeLists.txt:181), whose results are not reproducible
 * off an NVIDIA device.  libfovpt defines its results in terms of the functions below:
 * every one is evaluated in IEEE binary64 with +,-,*,/ and sqrt only (no fused
 * multiply-add: build with -ffp-contract=off) and rounded once to binary32, so the same
 * source gives the same bits under g++ on the host and under hipcc on gfx950.
 *
 * Accuracy.  Over its domain every function is within 0.5 + 2^-20 binary32 ulp of the true
 * value (the final rounding's half ulp plus the binary64 evaluation's error; an ulp below
 * 2^-126 counts as 2^-149), i.e. it agrees with a correctly rounded libm in all but a
 * vanishing fraction of arguments.  That bound is what tests/test_detmath_cpu.py and
 * tests/test_detmath_gpu.py assert against a high-precision reference; the measured maxima
 * are about 0.5 + 2^-23.
 *
 * Domains, and what is undefined (no function below checks for it -- they are inlined into
 * kernels and carry no branch for inputs the library never passes):
 *   fovpt_dm_sincos/sinf/cosf  |x| <= 2^20.  Larger or non-finite x: undefined.
 *   fovpt_dm_acosf             [-1, 1].  Outside (and NaN): undefined.
 *   fovpt_dm_atan2f            finite operands, signed zeros as C99 (atan2(+-0, -0) = +-pi).
 *                              An infinite or NaN operand: undefined.
 *   fovpt_dm_logf              every binary32: x < 0 -> NaN, +-0 -> -inf, +inf -> +inf, NaN -> NaN.
 *   fovpt_dm_powf              x >= 0 finite, any y.  In this order: a NaN operand -> NaN (also for
 *                              y = 0 or x = 1, unlike C99); y = 0 -> 1; x = +-0 -> +0 for y > 0, +inf
 *                              for y < 0 (-0 counts as +0); x < 0 -> NaN for every y (no integer-
 *                              exponent case); x = 1 -> 1; y = +-inf -> 0 or +inf as C99.  Results
 *                              overflow to +inf and underflow through the subnormals to +0.
 *                              x = +inf: undefined.
 *   fovpt_dm_floor             |x| < 2^51 (the callers above stay below 2^21 and 2^11).
 * "Undefined" means what it does in C: the conversions to integer inside differ between x86
 * and gfx950 there, so not even host/device agreement holds.
 *
 * Call sites in the reference: Probe.cuh:40-41,53-55,161 (acosf, atan2, sinf, cosf),
 * Disney.cuh:63 (logf), :216-217,293-294 (sinf, cosf), maths.h:250-251,261 (cosf, sinf),
 * cuda/helpers.h:38 (powf).
 */
#ifndef FOVPT_DETMATH_H
#define FOVPT_DETMATH_H

#include <stdint.h>

#if defined(__HIPCC__)
#define FOVPT_HD __host__ __device__ inline
#else
#define FOVPT_HD static inline
#endif

FOVPT_HD double fovpt_dm_bits2d(uint64_t u) { double d; __builtin_memcpy(&d, &u, 8); return d; }
FOVPT_HD uint64_t fovpt_dm_d2bits(double d) { uint64_t u; __builtin_memcpy(&u, &d, 8); return u; }
FOVPT_HD uint32_t fovpt_dm_f2bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }

/* floor for |x| < 2^51 without libm (beyond 2^63, and for NaN, the cast is undefined) */
FOVPT_HD double fovpt_dm_floor(double x)
{
    double t = (double)(long long)x;      /* truncation toward zero */
    return (t > x) ? t - 1.0 : t;
}

/* sin and cos of a binary32 argument, |x| <= 2^20 */
FOVPT_HD void fovpt_dm_sincos(float xf, float* s_out, float* c_out)
{
    const double x = (double)xf;
    const double kd = fovpt_dm_floor(x * 0.63661977236758138 + 0.5);
    const long long k = (long long)kd;
    /* x - k*pi/2 with pi/2 = P1 + P2 + P3 (to 2^-122): P1 and P2 carry 33 significant bits each, so kd*P1 and
     * kd*P2 are exact for kd < 2^20, x - kd*P1 is exact (a 24-bit and a 53-bit number that nearly cancel), and what
     * rounds after that is of the order 2^-53 |r|.  A 53-bit head instead makes the first product round and r wrong
     * by up to 2^-53 |x|: 12 ulp of the result at |x| = 256.  For every binary32 x in [0, 2 pi] the two reductions
     * give the same sin and cos bits. */
    const double p1 = 1.5707963267341256;          /* 0x1.921fb544p+0 (decimal: C++14 has no hexadecimal literals) */
    const double p2 = 6.077100506303966e-11;       /* 0x1.0b4611a6p-34 */
    const double p3 = 2.0222662487959506e-21;      /* 0x1.3198a2e037073p-69 */
    const double r = ((x - kd * p1) - kd * p2) - kd * p3;
    const double z = r * r;
    /* Taylor, |r| <= pi/4: truncation < 3e-14 relative */
    double ps = -1.0 / 1307674368000.0;            /* -1/15! */
    ps = ps * z + 1.0 / 6227020800.0;              /*  1/13! */
    ps = ps * z - 1.0 / 39916800.0;                /* -1/11! */
    ps = ps * z + 1.0 / 362880.0;                  /*  1/9!  */
    ps = ps * z - 1.0 / 5040.0;                    /* -1/7!  */
    ps = ps * z + 1.0 / 120.0;                     /*  1/5!  */
    ps = ps * z - 1.0 / 6.0;                       /* -1/3!  */
    const double sr = r + r * (z * ps);
    double pc = 1.0 / 20922789888000.0;            /*  1/16! */
    pc = pc * z - 1.0 / 87178291200.0;             /* -1/14! */
    pc = pc * z + 1.0 / 479001600.0;               /*  1/12! */
    pc = pc * z - 1.0 / 3628800.0;                 /* -1/10! */
    pc = pc * z + 1.0 / 40320.0;                   /*  1/8!  */
    pc = pc * z - 1.0 / 720.0;                     /* -1/6!  */
    pc = pc * z + 1.0 / 24.0;                      /*  1/4!  */
    pc = pc * z - 0.5;                             /* -1/2!  */
    const double cr = 1.0 + z * pc;
    double s, c;
    switch ((int)(k & 3)) {
    case 0:  s = sr;  c = cr;  break;
    case 1:  s = cr;  c = -sr; break;
    case 2:  s = -sr; c = -cr; break;
    default: s = -cr; c = sr;  break;
    }
    /* sin(-0) = -0 (a select, not a branch): above, r + r*(z*ps) adds two zeros of opposite sign, which gives +0 */
    *s_out = (xf == 0.0f) ? xf : (float)s;
    *c_out = (float)c;
}

FOVPT_HD float fovpt_dm_sinf(float x) { float s, c; fovpt_dm_sincos(x, &s, &c); return s; }
FOVPT_HD float fovpt_dm_cosf(float x) { float s, c; fovpt_dm_sincos(x, &s, &c); return c; }

/* atan of t in [0,1] (double in, double out) */
FOVPT_HD double fovpt_dm_atan01(double t)
{
    double base = 0.0;
    if (t > 0.41421356237309503) {       /* tan(pi/8): atan t = pi/4 + atan((t-1)/(t+1)) */
        t = (t - 1.0) / (t + 1.0);
        base = 0.78539816339744831;
    }
    const double z = t * t;
    /* odd Taylor series to t^29, |t| <= 0.4143: truncation < 1e-13 */
    double p = 1.0 / 29.0;
    p = -1.0 / 27.0 + z * p;  p = 1.0 / 25.0 + z * p;
    p = -1.0 / 23.0 + z * p;  p = 1.0 / 21.0 + z * p;
    p = -1.0 / 19.0 + z * p;  p = 1.0 / 17.0 + z * p;
    p = -1.0 / 15.0 + z * p;  p = 1.0 / 13.0 + z * p;
    p = -1.0 / 11.0 + z * p;  p = 1.0 / 9.0 + z * p;
    p = -1.0 / 7.0 + z * p;   p = 1.0 / 5.0 + z * p;
    p = -1.0 / 3.0 + z * p;
    return base + (t + t * (z * p));
}

/* atan2 on doubles, full quadrant handling (signed zeros as C99) */
FOVPT_HD double fovpt_dm_atan2d(double y, double x)
{
    const int yneg = (int)(fovpt_dm_d2bits(y) >> 63);
    const int xneg = (int)(fovpt_dm_d2bits(x) >> 63);
    const double ay = yneg ? -y : y;
    const double ax = xneg ? -x : x;
    double a;
    if (ax == 0.0 && ay == 0.0) a = 0.0;
    else if (ay <= ax)          a = fovpt_dm_atan01(ay / ax);
    else                        a = 1.5707963267948966 - fovpt_dm_atan01(ax / ay);
    if (xneg) a = 3.1415926535897931 - a;
    return yneg ? -a : a;
}

FOVPT_HD float fovpt_dm_atan2f(float y, float x) { return (float)fovpt_dm_atan2d((double)y, (double)x); }

/* acos of x in [-1,1] */
FOVPT_HD float fovpt_dm_acosf(float xf)
{
    const double x = (double)xf;
    const double s2 = (1.0 - x) * (1.0 + x);
    return (float)fovpt_dm_atan2d(__builtin_sqrt(s2), x);
}

/* natural log of a positive finite double */
FOVPT_HD double fovpt_dm_logd(double x)
{
    uint64_t b = fovpt_dm_d2bits(x);
    int e = (int)((b >> 52) & 0x7ff);
    if (e == 0) {                          /* subnormal double: rescale */
        x = x * 18014398509481984.0;       /* 2^54 */
        b = fovpt_dm_d2bits(x);
        e = (int)((b >> 52) & 0x7ff) - 54;
    }
    e -= 1023;
    double m = fovpt_dm_bits2d((b & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL);   /* [1,2) */
    if (m > 1.4142135623730951) { m = m * 0.5; e += 1; }
    const double s = (m - 1.0) / (m + 1.0);   /* |s| <= 0.1716 */
    const double z = s * s;
    double p = 1.0 / 21.0;
    p = 1.0 / 19.0 + z * p;  p = 1.0 / 17.0 + z * p;  p = 1.0 / 15.0 + z * p;
    p = 1.0 / 13.0 + z * p;  p = 1.0 / 11.0 + z * p;  p = 1.0 / 9.0 + z * p;
    p = 1.0 / 7.0 + z * p;   p = 1.0 / 5.0 + z * p;   p = 1.0 / 3.0 + z * p;
    const double lm = 2.0 * (s + s * (z * p));
    return (double)e * 0.69314718055994529 + lm;
}

FOVPT_HD float fovpt_dm_logf(float x)
{
    if (x != x) return x;
    if (x < 0.0f) return (float)fovpt_dm_bits2d(0x7ff8000000000000ULL);
    if (x == 0.0f) return (float)fovpt_dm_bits2d(0xfff0000000000000ULL);
    if (fovpt_dm_f2bits(x) == 0x7f800000u) return x;
    return (float)fovpt_dm_logd((double)x);
}

/* exp of a double in [-700, 700] */
FOVPT_HD double fovpt_dm_expd(double d)
{
    const double kd = fovpt_dm_floor(d * 1.4426950408889634 + 0.5);
    const double r = (d - kd * 0.69314718055994529) - kd * 2.3190468138462996e-17;
    /* Taylor to r^13, |r| <= 0.3466: truncation < 1e-17 */
    double p = 1.0 / 6227020800.0;
    p = 1.0 / 479001600.0 + r * p;  p = 1.0 / 39916800.0 + r * p;
    p = 1.0 / 3628800.0 + r * p;    p = 1.0 / 362880.0 + r * p;
    p = 1.0 / 40320.0 + r * p;      p = 1.0 / 5040.0 + r * p;
    p = 1.0 / 720.0 + r * p;        p = 1.0 / 120.0 + r * p;
    p = 1.0 / 24.0 + r * p;         p = 1.0 / 6.0 + r * p;
    p = 0.5 + r * p;
    const double er = 1.0 + (r + r * (r * p));
    const long long k = (long long)kd;
    return er * fovpt_dm_bits2d((uint64_t)(k + 1023) << 52);
}

/* powf for x >= 0 (the sRGB curve, cuda/helpers.h:37-38) */
FOVPT_HD float fovpt_dm_powf(float x, float y)
{
    if (x != x || y != y) return x + y;
    if (y == 0.0f) return 1.0f;
    if (x == 0.0f) return (y > 0.0f) ? 0.0f : (float)fovpt_dm_bits2d(0x7ff0000000000000ULL);
    if (x < 0.0f) return (float)fovpt_dm_bits2d(0x7ff8000000000000ULL);
    if (x == 1.0f) return 1.0f;
    double d = (double)y * fovpt_dm_logd((double)x);
    if (d > 700.0) d = 700.0;
    if (d < -700.0) d = -700.0;
    return (float)fovpt_dm_expd(d);
}

#endif /* FOVPT_DETMATH_H */
