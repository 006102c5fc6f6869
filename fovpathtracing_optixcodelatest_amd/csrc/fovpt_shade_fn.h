// fovpt_shade_fn.h -- the device functions of a shaded hit: the path's random numbers, the probe (Probe.cuh) and the Disney
// BSDF (Disney.cuh).  k_shade and k_generate (wavefront.hip) are their callers in a frame; shade_debug.hip hands them chosen
// inputs one at a time (fovpt_debug_probe_sample / _probe_eval / _bsdf) from a translation unit of its own, so that a second
// caller cannot change an inlining decision inside k_shade.
#ifndef FOVPT_SHADE_FN_H
#define FOVPT_SHADE_FN_H
#include "fovpt_device.h"
#include "../../include/fovpt_detmath.h"
#include "fovpt_pixel.h"            // V3 and its operators, clampf, lerpf

namespace {

#define kPi (3.141592653589793f)
#define k2Pi (3.141592653589793f * 2.0f)
#define kInvPi (1.0f / kPi)
#define kInv2Pi (1.0f / k2Pi)

// ------------------------------------------------------------------------------------------
// RNG (cuda/random.h:34-59,101-104; maths.h:170-227)
// ------------------------------------------------------------------------------------------
__device__ inline uint32_t tea4(uint32_t v0, uint32_t v1)
{
    uint32_t s0 = 0;
#pragma unroll
    for (int n = 0; n < 4; n++) {
        s0 += 0x9e3779b9u;
        v0 += ((v1 << 4) + 0xa341316cu) ^ (v1 + s0) ^ ((v1 >> 5) + 0xc8013ea4u);
        v1 += ((v0 << 4) + 0xad90777du) ^ (v0 + s0) ^ ((v0 >> 5) + 0x7e95761eu);
    }
    return v0;
}
__device__ inline float rnd(uint32_t& prev)
{
    prev = 1664525u * prev + 1013904223u;
    return (float)(prev & 0x00FFFFFFu) / (float)0x01000000;
}
struct Rng {
    uint32_t s1, s2;
    __device__ inline uint32_t next()
    {
        s1 = (s2 ^ ((s1 << 5) | (s1 >> 27))) ^ (s1 * s2);
        s2 = s1 ^ ((s2 << 12) | (s2 >> 20));
        return s1;
    }
    __device__ inline float randf()
    {
        // maths.h:199-210: value * (1/float(0xffffffff)), clamp to [0, 0.999999]
        return clampf((float)next() * (1.0f / 4294967296.0f), 0.f, 0.999999f);
    }
    __device__ inline float randf01()      // Randf(0,1), maths.h:213-217
    {
        float t = randf();
        return (1.0f - t) * 0.0f + t * 1.0f;
    }
};

// ------------------------------------------------------------------------------------------
// Probe (Probe.cuh)
// ------------------------------------------------------------------------------------------
__device__ inline void probe_dir_to_uv(const V3& dir, float& u, float& v)     // :38-46
{
    float theta = fovpt_dm_acosf(clampf(dir.y, -1.0f, 1.0f));
    float phi = (dir.x == 0.0f && dir.z == 0.0f) ? 0.0f : fovpt_dm_atan2f(dir.z, dir.x);
    u = (kPi + phi) * kInvPi * 0.5f;
    v = theta * kInvPi;
}
// row_mul is 1, or 0 when every row of the probe (texels and row tables) is bit-identical to row 0 -- the
// reference's shipped lighting is such a probe (loadColor, main.cpp:175-187) -- so that all lookups land in
// one L1-resident row instead of 8-33 MB of HBM/L2.  Same values either way.
__device__ inline float4 probe_eval(const fovpt_probe& pr, int row_mul, float u, float v)  // :61-67
{
    int px = max(0, min((int)(u * pr.width), pr.width - 1));
    int py = max(0, min((int)(v * pr.height), pr.height - 1));
    return ((const float4*)pr.data)[py * row_mul * pr.width + px];
}
__device__ inline int lower_bound(const float* __restrict__ a, int lower, int upper, float value)   // :119-136
{
    while (lower < upper) {
        int mid = lower + (upper - lower) / 2;
        if (a[mid] < value) lower = mid + 1;
        else upper = mid;
    }
    return lower;
}
// lower_bound through a guide table: G[m] = lower_bound(a, w_m), w_m = fl(m * fl(1/n)), m = 0..n+1 (relative to the
// start of the segment).  w_m is non-decreasing in m and lower_bound is monotone in its value, so for the m with
// w_m <= r < w_(m+1) the answer lies in [G[m], G[m+1]]: one or two candidates on a typical environment map, where the
// reference's search does log2(n) dependent loads.  m = int(r n) is off by at most one from that bracket (the products
// carry relative errors of 1e-7); it is corrected with two multiplications, and if the bracket still does not hold the
// whole segment is searched.  On a sorted array lower_bound is unique, so the result is the one the reference's full
// search returns (Probe.cuh:119-136); fovpt_set_probe only enables the tables after checking that the CDFs are
// non-decreasing.  (r1 bracketed with [G[m-1], G[m+2]]: three candidates on average, and more than four -- a divergent
// dependent search for the whole wave -- in 27 % of the row and 11 % of the column lookups on an HDR map: the shading
// launches took 0.315 instead of 0.229 ms per frame with a 1920x1080 HDR sky.)
// STRIDE: distance of consecutive array elements in floats (1: a plain CDF array; 8: the cdf member of the packed records)
template <int STRIDE>
__device__ inline int lower_bound_guided(const float* __restrict__ a, const uint32_t* __restrict__ guide, int base, int n, float value)
{
    const float fn = (float)n, inv = 1.0f / fn;
    int k = (int)(value * fn);
    k = max(0, min(k, n - 1));
    if ((float)k * inv > value) k = max(k - 1, 0);
    else if ((float)(k + 1) * inv <= value) k = min(k + 1, n - 1);
    const bool bracket = (float)k * inv <= value && value < (float)(k + 1) * inv;
    int lower = base + (bracket ? (int)guide[k] : 0);
    int upper = base + (bracket ? (int)guide[k + 1] : n);
    // A handful of candidates (the usual case): fetch them side by side instead of one after the other.
    // On a non-decreasing array the elements below `value` are a prefix of the range, so their number is
    // the offset the binary search would find.
    const int m = upper - lower;
    if (m <= 4) {
        if (m <= 0) return lower;
        const int last = upper - 1;
        const float v0 = a[(size_t)lower * STRIDE], v1 = a[(size_t)min(lower + 1, last) * STRIDE], v2 = a[(size_t)min(lower + 2, last) * STRIDE],
                    v3 = a[(size_t)min(lower + 3, last) * STRIDE];
        return lower + (int)(v0 < value) + (int)(m > 1 && v1 < value) + (int)(m > 2 && v2 < value) + (int)(m > 3 && v3 < value);
    }
    while (lower < upper) {
        int mid = lower + (upper - lower) / 2;
        if (a[(size_t)mid * STRIDE] < value) lower = mid + 1;
        else upper = mid;
    }
    return lower;
}
// rec: per texel one 32-byte record {cdfX, pdfX, r, g, b, -, -, -} (built at setProbe next to the guide tables, or null).
// The column search, the pdf and the colour of a sample then come from one or two cache lines instead of four arrays: on a
// 1920x1080 HDR map (58 MB of tables, nothing of it in L1) every lookup of the split layout is its own miss.
// DRAW: where the two numbers come from -- the path's stream (Rng, as ProbeSample draws them), or a pair the caller chose
// (shade_debug.hip), which also takes the row and column the searches found.
template <class DRAW>
__device__ inline void probe_sample(const fovpt_probe& pr, const uint32_t* __restrict__ guide_x, const uint32_t* __restrict__ guide_y, const float4* __restrict__ rec,
                                    int row_mul, V3& dir, V3& color, float& pdf, DRAW& rng, int* row_out = nullptr, int* col_out = nullptr)   // :138-169
{
    float r1 = rng.randf01();
    float r2 = rng.randf01();
    int row, col;
    if (guide_x) {
        row = lower_bound_guided<1>(pr.cdfValuesY, guide_y, 0, pr.height, r1);
        const int rx = row * row_mul;
        if (rec) col = lower_bound_guided<8>((const float*)rec, guide_x + (size_t)rx * (pr.width + 2), rx * pr.width, pr.width, r2) - rx * pr.width;
        else col = lower_bound_guided<1>(pr.cdfValuesX, guide_x + (size_t)rx * (pr.width + 2), rx * pr.width, pr.width, r2) - rx * pr.width;
    } else {
        row = lower_bound(pr.cdfValuesY, 0, pr.height, r1);
        const int rx = row * row_mul;
        col = lower_bound(pr.cdfValuesX, rx * pr.width, (rx + 1) * pr.width, r2) - rx * pr.width;
    }
    const int rowx = row * row_mul;
    if (guide_x && rec) {
        const float4 ra = rec[2 * (size_t)(rowx * pr.width + col)], rb = rec[2 * (size_t)(rowx * pr.width + col) + 1];
        color = v3(ra.z, ra.w, rb.x);
        pdf = ra.y * pr.pdfValuesY[row];
    } else {
        color = v3(((const float4*)pr.data)[rowx * pr.width + col]);
        pdf = pr.pdfValuesX[rowx * pr.width + col] * pr.pdfValuesY[row];
    }
    float u = col / float(pr.width);
    float v = row / float(pr.height);
    float sinTheta, cosTheta;
    fovpt_dm_sincos(v * kPi, &sinTheta, &cosTheta);
    if (sinTheta == 0.0f) pdf = 0.0f;
    else pdf *= pr.width * pr.height / (2.0f * kPi * kPi * sinTheta);
    // ProbeUVToDir :48-58 (theta = v*kPi is the same value as above)
    float sinPhi, cosPhi;
    fovpt_dm_sincos(u * 2.0f * kPi, &sinPhi, &cosPhi);
    dir = v3(-sinTheta * cosPhi, cosTheta, -sinTheta * sinPhi);
    if (row_out) { *row_out = row; *col_out = col; }
}

// ------------------------------------------------------------------------------------------
// Disney BSDF (Disney.cuh)
// ------------------------------------------------------------------------------------------
typedef fovpt_material Mat;

// The reference writes 1.0 / sqrtf(x) and 0.5 + y with binary64 literals: a binary64 operation on binary32 values, rounded back to
// binary32.  That equals the correctly rounded binary32 operation (rounding twice is innocuous for + - * / sqrt when the wide format
// has at least 2 * 24 + 2 significant bits), which is how the compiler emits them: no binary64 instruction comes from these lines
// (the 231 of k_shade are the polynomial cores of include/fovpt_detmath.h).  FOVPT_OP_RSQRTD / _HALFPLUS check the device's result
// against the oracle's binary64 expression over every binade (tests/test_gpu_parity.py).
__device__ inline float rcp_of_sqrt_as_the_reference(float x) { return (float)(1.0 / (double)sqrtf(x)); }
__device__ inline void basis_from_vector(const V3& w, V3& u, V3& v)          // maths.h:94-108
{
    if (fabsf(w.x) > fabsf(w.y)) {
        float invLen = rcp_of_sqrt_as_the_reference(w.x * w.x + w.z * w.z);
        u = v3(-w.z * invLen, 0.0f, w.x * invLen);
    } else {
        float invLen = rcp_of_sqrt_as_the_reference(w.y * w.y + w.z * w.z);
        u = v3(0.0f, w.z * invLen, -w.y * invLen);
    }
    v = cross(w, u);
}
__device__ inline V3 safe_normalize(const V3& a)                              // maths.h:144-156
{
    float m = dot(a, a);
    if ((double)m > 0.0) return a * rcp_of_sqrt_as_the_reference(m);
    return v3(0.0f);
}
__device__ inline float half_plus_as_the_reference(float y) { return (float)(0.5 + (double)y); }      // (see rcp_of_sqrt_as_the_reference)
__device__ inline float schlick(float u)                                      // Disney.cuh:51-56
{
    float m = clampf(1 - u, 0.0f, 1.0f);
    float m2 = m * m;
    return m2 * m2 * m;
}
__device__ inline float gtr1_pre(float NDotH, float a2, float log_a2)         // GTR1 :58-64 with a*a and log(a*a) given (a2 < 0: a >= 1)
{
    if (a2 < 0.0f) return kInvPi;
    float t = 1 + (a2 - 1) * NDotH * NDotH;
    return (a2 - 1) / (kPi * log_a2 * t);
}
__device__ inline float gtr2(float NDotH, float a)                            // :66-71
{
    float a2 = a * a;
    float t = 1.0f + (a2 - 1.0f) * NDotH * NDotH;
    return a2 / (kPi * t * t);
}
__device__ inline float smith_ggx(float NDotv, float alphaG)                  // :73-78
{
    float a = alphaG * alphaG;
    float b = NDotv * NDotv;
    return 1 / (NDotv + sqrtf(a + b - a * b));
}
__device__ inline float fresnel(float VDotN, float etaI, float etaT)          // Fr, :81-98
{
    float SinThetaT2 = sqr(etaI / etaT) * (1.0f - VDotN * VDotN);
    if (SinThetaT2 > 1.0f) return 1.0f;
    float LDotN = sqrtf(1.0f - SinThetaT2);
    float eta = etaT / etaI;
    float r1 = (VDotN - eta * LDotN) / (VDotN + eta * LDotN);
    float r2 = (LDotN - eta * VDotN) / (LDotN + eta * VDotN);
    return 0.5f * (sqr(r1) + sqr(r2));
}
// Terms of BSDFPdf / BSDFSample / BSDFEval that depend on the hit and the view direction only.  A hit
// evaluates the BSDF for two light directions (the probe sample and the BSDF sample) and its pdf for
// both: the reference recomputes these terms every time, here they are computed once -- the same
// expressions on the same operands, hence the same bits.
struct BsdfView {
    float etaI, etaO;
    float NDotV;          // dot(N, V)
    float FrV;            // Fr(dot(N, V), etaI, etaO)                       :154, :199, :340
    float a;              // max(0.001, roughness)
    float GV_a, GV_q;     // SmithGGX(NDotV, a), SmithGGX(NDotV, 0.25)       :350, :375, :383
    float FV;             // SchlickFresnel(NDotV)                           :362, :378
    V3 Cspec0;            // :330-334
    float cc_a2, cc_log;  // clearcoat GTR1: a = mix(.1, .001, clearcoatGloss); a*a and log(a*a)    :381, :58-64
};
__device__ inline BsdfView bsdf_view(const Mat& mat, const V3& albedo, float etaI, float etaO, const V3& N, const V3& V)
{
    BsdfView w;
    w.etaI = etaI; w.etaO = etaO;
    w.NDotV = dot(N, V);
    w.FrV = fresnel(w.NDotV, etaI, etaO);
    w.a = fmaxf(0.001f, mat.roughness);
    w.GV_a = smith_ggx(w.NDotV, w.a);
    w.GV_q = smith_ggx(w.NDotV, .25f);
    w.FV = schlick(w.NDotV);
    const V3 Cdlin = albedo;
    const float Cdlum = (float)(.3 * (double)Cdlin.x + .6 * (double)Cdlin.y + .1 * (double)Cdlin.z);
    const V3 Ctint = Cdlum > 0.0f ? div_vs(Cdlin, Cdlum) : v3(1.0f);
    w.Cspec0 = lerp3((float)((double)mat.specular * .08) * lerp3(v3(1.0f), Ctint, mat.specularTint), Cdlin, mat.metallic);
    const float cc_a = lerpf(.1f, .001f, mat.clearcoatGloss);
    w.cc_a2 = cc_a >= 1 ? -1.0f : cc_a * cc_a;                  // -1: GTR1 returns 1/pi (a >= 1)
    w.cc_log = cc_a >= 1 ? 0.0f : fovpt_dm_logf(w.cc_a2);
    return w;
}
__device__ float bsdf_pdf(const Mat& mat, const BsdfView& w, const V3& n, const V3& V, const V3& L)   // :152-193
{
    if (dot(L, n) <= 0.0f) {
        float bsdfPdf = 0.0f;
        float brdfPdf = kInv2Pi * mat.subsurface * 0.5f;
        return lerpf(brdfPdf, bsdfPdf, mat.transmission);
    }
    const float F = w.FrV;
    const float a = w.a;
    const V3 half = safe_normalize(L + V);
    const float cosThetaHalf = fabsf(dot(half, n));
    const float pdfHalf = gtr2(cosThetaHalf, a) * cosThetaHalf;
    float pdfSpec = 0.25f * pdfHalf / fmaxf(1.e-6f, dot(L, half));
    float pdfDiff = fabsf(dot(L, n)) * kInvPi * (1.0f - mat.subsurface);
    float bsdfPdf = pdfSpec * F;
    float brdfPdf = lerpf(pdfDiff, pdfSpec, 0.5f);
    return lerpf(brdfPdf, bsdfPdf, mat.transmission);
}
// returns pdf; light = sampled direction.
// The lanes of a wave take different branches of BSDFSample, and three of the four end in the same
// work: one sincos and a change of basis.  The random numbers are drawn in the reference's order and
// the branch is remembered; the sincos and (for both "sample specular" branches, Disney.cuh:211-226
// and :287-307) the GGX half vector are then evaluated once for all lanes.
__device__ float bsdf_sample(const Mat& mat, const BsdfView& w, const V3& U, const V3& V, const V3& N,
                             const V3& view, V3& light, Rng& rng)             // :197-315
{
    enum { SPECULAR, UNIFORM, COSINE };
    int kind;
    float r1, r2, z = 0.0f, angle;
    if (rng.randf() < mat.transmission) {
        const float F = w.FrV;
        if (rng.randf() < F) {
            r1 = rng.randf01();
            r2 = rng.randf01();
            kind = SPECULAR;
        } else {
            // Refract, :36-49
            float eta = w.etaI / w.etaO;
            float cosThetaI = w.NDotV;
            float sin2ThetaI = fmaxf(0.0f, 1.0f - cosThetaI * cosThetaI);
            float sin2ThetaT = eta * eta * sin2ThetaI;
            if (sin2ThetaT >= 1) return 0.0f;
            float cosThetaT = sqrtf(1.0f - sin2ThetaT);
            light = eta * neg(view) + (eta * cosThetaI - cosThetaT) * N;
            return (1.0f - F) * mat.transmission;
        }
    } else {
        r1 = rng.randf01();
        r2 = rng.randf01();
        if (rng.randf() < 0.5f) {
            if (rng.randf() < mat.subsurface) { kind = UNIFORM; z = rng.randf01(); }
            else kind = COSINE;
        } else {
            kind = SPECULAR;
        }
    }
    if (kind == SPECULAR) angle = r1 * k2Pi;                   // phiHalf
    else if (kind == COSINE) angle = k2Pi * r2;                // theta, maths.h:262
    else angle = k2Pi * rng.randf01();                         // phi, maths.h:248
    float sn, cs;
    fovpt_dm_sincos(angle, &sn, &cs);
    if (kind == SPECULAR) {
        const float a = w.a;
        const float cosThetaHalf = sqrtf((1.0f - r2) / (1.0f + (sqr(a) - 1.0f) * r2));
        const float sinThetaHalf = sqrtf(fmaxf(0.0f, 1.0f - sqr(cosThetaHalf)));
        V3 half = U * (sinThetaHalf * cs) + V * (sinThetaHalf * sn) + N * cosThetaHalf;
        if (dot(half, view) <= 0.0f) half = half * -1.0f;
        light = 2.0f * dot(view, half) * half - view;
    } else if (kind == UNIFORM) {
        // UniformSampleHemisphere, maths.h:243-254
        const float ww = sqrtf(1.0f - z * z);
        const float x = cs * ww, y = sn * ww;
        light = U * x + V * y - N * z;
    } else {
        // CosineSampleHemisphere, maths.h:256-277
        const float r = sqrtf(r1);
        const float sx = r * cs, sy = r * sn;
        const float zz = sqrtf(fmaxf(0.0f, 1.0f - sx * sx - sy * sy));
        light = U * sx + V * sy + N * zz;
    }
    return bsdf_pdf(mat, w, N, view, light);
}
__device__ V3 bsdf_eval(const Mat& mat, const V3& albedo, const BsdfView& w, const V3& N, const V3& V, const V3& L)   // :318-427
{
    float NDotL = dot(N, L);
    const float NDotV = w.NDotV;
    V3 H = normalize(L + V);
    float NDotH = dot(N, H);
    float LDotH = dot(L, H);
    const V3 Cdlin = albedo;
    const V3 Cspec0 = w.Cspec0;
    V3 bsdf = v3(0.0f);
    V3 brdf = v3(0.0f);
    // both lobes use the same D and G terms on the upper hemisphere (:346-351 and :371-376)
    float Ds = 0.0f, Gs = 0.0f;
    if (NDotL > 0) {
        Ds = gtr2(NDotH, w.a);
        Gs = w.GV_a * smith_ggx(NDotL, w.a);
    }
    if (mat.transmission > 0.0f) {
        if (NDotL <= 0) {
            const float F = w.FrV;
            bsdf = v3(mat.transmission * (1.0f - F) / fabsf(NDotL) * (1.0f - mat.metallic));
        } else {
            float FH = fresnel(LDotH, w.etaI, w.etaO);
            V3 Fs = lerp3(Cspec0, v3(1.0f), FH);
            bsdf = Gs * Fs * Ds;
        }
    }
    if (mat.transmission < 1.0f) {
        if (NDotL <= 0) {
            if (mat.subsurface > 0.0f) {
                V3 s = v3(sqrtf(mat.color.x), sqrtf(mat.color.y), sqrtf(mat.color.z));
                float FL = schlick(fabsf(NDotL)), FV = w.FV;
                float Fd = (1.0f - 0.5f * FL) * (1.0f - 0.5f * FV);
                brdf = kInvPi * s * mat.subsurface * Fd * (1.0f - mat.metallic);
            }
        } else {
            float FH = schlick(LDotH);
            V3 Fs = lerp3(Cspec0, v3(1.f), FH);
            float FL = schlick(NDotL), FV = w.FV;
            float Fd90 = half_plus_as_the_reference(2.0f * LDotH * LDotH * mat.roughness);     // Disney.cuh: 0.5 + (binary32 product), in binary64
            float Fd = lerpf(1.0f, Fd90, FL) * lerpf(1.0f, Fd90, FV);
            float Dr = gtr1_pre(NDotH, w.cc_a2, w.cc_log);
            float Fc = lerpf(.04f, 1.0f, FH);
            float Gr = smith_ggx(NDotL, .25f) * w.GV_q;
            brdf = add_vs(kInvPi * Fd * Cdlin * (1.0f - mat.metallic) * (1.0f - mat.subsurface) + Gs * Fs * Ds,
                          mat.clearcoat * Gr * Fc * Dr);
        }
    }
    (void)NDotV;
    return lerp3(brdf, bsdf, mat.transmission);
}

}  // namespace

#endif  // FOVPT_SHADE_FN_H
