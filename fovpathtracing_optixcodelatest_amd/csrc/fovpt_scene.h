// fovpt_scene.h -- device access to the scene, shared by the wavefront kernels (wavefront.hip) and the G-buffer of
// fovpt_gbuffer (reconstruct.hip): triangle records in leaf order and the bilinear texture fetch of the shading kernel.
#pragma once

#include "fovpt_device.h"

namespace {

// triangle records: Moeller-Trumbore on them is in leaf_finish (traverse.hip), in the operation order of the parity contract
// (oracle intersect_tri)
__device__ inline TriRec load_tri_off(const TriRec* __restrict__ tris, uint32_t byte_off)
{
    const float4* p = (const float4*)((const char*)tris + byte_off);
    const float4 a = p[0], b = p[1], c = p[2];
    TriRec T;
    T.v0x = a.x; T.v0y = a.y; T.v0z = a.z; T.e1x = a.w;
    T.e1y = b.x; T.e1z = b.y; T.e2x = b.z; T.e2y = b.w;
    T.e2z = c.x; T.prim = __float_as_uint(c.y); T.mesh = __float_as_uint(c.z); T.pad = 0;
    return T;
}

// (float)c / 255.0f for c = 0..255 without the division sequence: one Newton step on q = c * fl(1/255)
// with fused multiply-adds gives the correctly rounded quotient for every one of the 256 inputs
// (checked exhaustively: test_unorm8_device_matches_division, FOVPT_OP_UNORM8)
__device__ inline float unorm8(uint32_t c)
{
    const float f = (float)c, r = 1.0f / 255.0f;
    const float q = f * r;
    return __builtin_fmaf(__builtin_fmaf(-q, 255.0f, f), r, q);
}
__device__ inline float4 tex_unpack(uint32_t p)
{
    return make_float4(unorm8(p & 255u), unorm8((p >> 8) & 255u), unorm8((p >> 16) & 255u), unorm8(p >> 24));
}
// floor-mod of a texel coordinate (wrap addressing); a power-of-two size needs no division
__device__ inline int tex_wrap(int x, int n)
{
    if ((n & (n - 1)) == 0) return x & (n - 1);
    x %= n;
    return x < 0 ? x + n : x;
}
// bilinear, wrap, normalized coordinates (the fp32 contract standing in for tex2D<float4>, :664)
__device__ inline float4 tex2d(const TexDev& T, float u, float v)
{
    const float x = u * (float)T.w - 0.5f, y = v * (float)T.h - 0.5f;
    const float fx0 = floorf(x), fy0 = floorf(y);
    const float fx = x - fx0, fy = y - fy0;
    const int x0 = tex_wrap((int)fmaxf(-1.0e9f, fminf(1.0e9f, fx0)), T.w), y0 = tex_wrap((int)fmaxf(-1.0e9f, fminf(1.0e9f, fy0)), T.h);
    const int x1 = x0 + 1 == T.w ? 0 : x0 + 1, y1 = y0 + 1 == T.h ? 0 : y0 + 1;
    const uint32_t* r0 = T.px + (size_t)y0 * T.w;
    const uint32_t* r1 = T.px + (size_t)y1 * T.w;
    const float4 c00 = tex_unpack(r0[x0]), c10 = tex_unpack(r0[x1]), c01 = tex_unpack(r1[x0]), c11 = tex_unpack(r1[x1]);
    const float w00 = (1.0f - fx) * (1.0f - fy), w10 = fx * (1.0f - fy), w01 = (1.0f - fx) * fy, w11 = fx * fy;
    return make_float4(w00 * c00.x + w10 * c10.x + w01 * c01.x + w11 * c11.x,
                       w00 * c00.y + w10 * c10.y + w01 * c01.y + w11 * c11.y,
                       w00 * c00.z + w10 * c10.z + w01 * c01.z + w11 * c11.z,
                       w00 * c00.w + w10 * c10.w + w01 * c01.w + w11 * c11.w);
}

}  // namespace
