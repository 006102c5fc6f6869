// shade_debug.hip -- test hooks: the device functions of a shaded hit on inputs the caller chose, one thread per input.
//
// A frame draws the inputs of probe_sample, bsdf_sample and tex2d from the path's random stream and the scene, so the inputs on
// which the arguments in fovpt_shade_fn.h could break (a number bit-equal to a guide abscissa or a CDF entry, flat CDF runs,
// N.V = 0, roughness 0, total internal reflection, L = -V, texel boundaries, non-finite coordinates) reach k_shade by chance or
// never.  The kernels here call the SAME functions -- fovpt_shade_fn.h and fovpt_scene.h, nothing restated -- and write what
// they return (fovpt_debug_probe_sample / _probe_eval / _bsdf / _tex2d, fovpt_api.hip).  They live in a translation unit of
// their own so that k_shade keeps its single caller of every one of these functions, and with it its inlining and its code.
// Not hot: no entry in check_resources.py.
#include "fovpt_shade_fn.h"
#include "fovpt_scene.h"

namespace {

// the two numbers of a probe sample, in the order ProbeSample draws them
struct GivenPair {
    float r1, r2;
    int drawn;
    __device__ inline float randf01() { return drawn++ == 0 ? r1 : r2; }
};

// out7: dir.xyz, color.xyz, pdf
__global__ __launch_bounds__(256) void k_debug_probe_sample(const fovpt_probe pr, const uint32_t* __restrict__ guide_x, const uint32_t* __restrict__ guide_y,
                                                            const float4* __restrict__ rec, int row_mul, int n, const float2* __restrict__ r12,
                                                            int2* __restrict__ rowcol, float* __restrict__ out7)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    GivenPair given;
    given.r1 = r12[i].x; given.r2 = r12[i].y; given.drawn = 0;
    V3 dir, color;
    float pdf;
    int row, col;
    probe_sample(pr, guide_x, guide_y, rec, row_mul, dir, color, pdf, given, &row, &col);
    rowcol[i] = make_int2(row, col);
    float* o = out7 + 7 * (size_t)i;
    o[0] = dir.x; o[1] = dir.y; o[2] = dir.z; o[3] = color.x; o[4] = color.y; o[5] = color.z; o[6] = pdf;
}

// the backplate of generate_rays; out6: u, v, texel.xyzw
__global__ __launch_bounds__(256) void k_debug_probe_eval(const fovpt_probe pr, int row_mul, int n, const float* __restrict__ dir3, float* __restrict__ out6)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 dir = v3(dir3[3 * (size_t)i], dir3[3 * (size_t)i + 1], dir3[3 * (size_t)i + 2]);
    float u, v;
    probe_dir_to_uv(dir, u, v);
    const float4 t = probe_eval(pr, row_mul, u, v);
    float* o = out6 + 6 * (size_t)i;
    o[0] = u; o[1] = v; o[2] = t.x; o[3] = t.y; o[4] = t.z; o[5] = t.w;
}

// in16: N.xyz, view.xyz, albedo.xyz, etaI, etaO, seed (bits), L_given.xyz, -
// out16: light.xyz, pdf, eval.xyz, pdf_again, rng_after s1 s2 (bits), eval_given.xyz, pdf_given, -, -
__global__ __launch_bounds__(256) void k_debug_bsdf(const Mat mat, int n, const float* __restrict__ in16, float* __restrict__ out16)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* a = in16 + 16 * (size_t)i;
    const V3 N = v3(a[0], a[1], a[2]), view = v3(a[3], a[4], a[5]), albedo = v3(a[6], a[7], a[8]), L_given = v3(a[12], a[13], a[14]);
    const float etaI = a[9], etaO = a[10];
    const uint32_t seed = __float_as_uint(a[11]);
    V3 bu, bv;
    basis_from_vector(N, bu, bv);
    const BsdfView w = bsdf_view(mat, albedo, etaI, etaO, N, view);
    Rng rng;                                       // Random(seed), as generate_rays seeds it
    rng.s1 = 315645664u + seed;
    rng.s2 = rng.s1 ^ 0x13ab45feu;
    V3 light = v3(0.f);
    const float pdf = bsdf_sample(mat, w, bu, bv, N, view, light, rng);
    V3 f = v3(0.f);
    float pdf_again = 0.f;
    if (pdf > 0.0f) {
        f = bsdf_eval(mat, albedo, w, N, view, light);
        pdf_again = bsdf_pdf(mat, w, N, view, light);
    }
    // the next-event branch of k_shade: the direction comes from the probe and may lie below the surface
    const float pdf_given = bsdf_pdf(mat, w, N, view, L_given);
    const V3 f_given = bsdf_eval(mat, albedo, w, N, view, L_given);
    float* o = out16 + 16 * (size_t)i;
    o[0] = light.x; o[1] = light.y; o[2] = light.z; o[3] = pdf;
    o[4] = f.x; o[5] = f.y; o[6] = f.z; o[7] = pdf_again;
    o[8] = __uint_as_float(rng.s1); o[9] = __uint_as_float(rng.s2);
    o[10] = f_given.x; o[11] = f_given.y; o[12] = f_given.z; o[13] = pdf_given;
    o[14] = 0.f; o[15] = 0.f;
}

__global__ __launch_bounds__(256) void k_debug_tex2d(const TexDev* __restrict__ textures, int texture, int n, const float2* __restrict__ uv, float4* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = tex2d(textures[texture], uv[i].x, uv[i].y);
}

inline unsigned blocks_of(int n) { return (unsigned)((n + 255) / 256); }

}  // namespace

void fovpt_launch_debug_probe_sample(hipStream_t st, const fovpt_probe& pr, const uint32_t* guide_x, const uint32_t* guide_y, const float4* rec, int row_mul,
                                     int n, const float2* r12, int2* rowcol, float* out7)
{
    hipLaunchKernelGGL(k_debug_probe_sample, dim3(blocks_of(n)), dim3(256), 0, st, pr, guide_x, guide_y, rec, row_mul, n, r12, rowcol, out7);
}
void fovpt_launch_debug_probe_eval(hipStream_t st, const fovpt_probe& pr, int row_mul, int n, const float* dir3, float* out6)
{
    hipLaunchKernelGGL(k_debug_probe_eval, dim3(blocks_of(n)), dim3(256), 0, st, pr, row_mul, n, dir3, out6);
}
void fovpt_launch_debug_bsdf(hipStream_t st, const fovpt_material& mat, int n, const float* in16, float* out16)
{
    hipLaunchKernelGGL(k_debug_bsdf, dim3(blocks_of(n)), dim3(256), 0, st, mat, n, in16, out16);
}
void fovpt_launch_debug_tex2d(hipStream_t st, const TexDev* textures, int texture, int n, const float2* uv, float4* out)
{
    hipLaunchKernelGGL(k_debug_tex2d, dim3(blocks_of(n)), dim3(256), 0, st, textures, texture, n, uv, out);
}
