// reconstruct.hip -- fovpt_gbuffer: a full-resolution primary-visibility G-buffer, and fovpt_reconstruct: the upsampling of
// a foveated frame's block-filled middle ring and periphery that it guides (cf. Weier et al. 2016, Koskela et al. 2019).
//
//   k_gbuffer_rays   one camera ray per pixel, the expression of generate_rays (wavefront.hip) with jitter 0.5, into queue 0
//                    (shard 0); the production k_traverse traces them in closest-hit mode (fovpt_launch_traverse)
//   k_gbuffer_fill   hit record -> primitive id, position and t, face-forwarded normal and albedo, as k_shade computes them
//   k_reconstruct    per block-filled pixel: the 3 x 3 anchors of its fill's lattice around its own block's anchor, weighted by
//                    a tent in pixel distance, normal and plane-distance edge stopping on the G-buffer; illumination
//                    (colour / rendered albedo) is interpolated and remodulated with the pixel's own G-buffer albedo
//
// One thread per pixel, 64 x 4 pixel tiles.  The reconstruction's definition, operation by operation, is
// tests/reconstruct_ref.py; -ffp-contract=off keeps every product and sum of it a separate binary32 op.
#include "fovpt_device.h"
#include "fovpt_pixel.h"
#include "fovpt_scene.h"

namespace {

__global__ __launch_bounds__(FOVPT_BLOCK) void k_gbuffer_rays(const FrameDev fd, RayQueue q, Counters* __restrict__ cnt)
{
    const uint32_t x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const uint32_t n = (uint32_t)fd.w * (uint32_t)fd.h;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < FOVPT_SHARDS)      // every ray in shard 0 of iteration 0's queue
        cnt->shard[threadIdx.x][FOVPT_CNT_Q(0)] = threadIdx.x == 0 ? n : 0u;
    if (x >= (uint32_t)fd.w || y >= (uint32_t)fd.h) return;
    const uint32_t idx = y * (uint32_t)fd.w + x;
    const float dx = 2.0f * (((float)x + 0.5f) / (float)fd.w) - 1.0f;       // generate_rays with jx = jy = 0.5
    const float dy = 2.0f * (((float)y + 0.5f) / (float)fd.h) - 1.0f;
    const V3 U = v3(fd.U[0], fd.U[1], fd.U[2]), V = v3(fd.V[0], fd.V[1], fd.V[2]), W = v3(fd.W[0], fd.W[1], fd.W[2]);
    const V3 dir = normalize(dx * U + dy * V + W);
    q.o[idx] = make_float4(fd.eye[0], fd.eye[1], fd.eye[2], __uint_as_float(idx));
    q.d[idx] = f4(dir, 0.f);
}

__global__ __launch_bounds__(FOVPT_BLOCK) void k_gbuffer_fill(const FrameDev fd, SceneView sc, RayQueue q, const float4* __restrict__ hits,
                                                              GBufferDev g)
{
    const uint32_t x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= (uint32_t)fd.w || y >= (uint32_t)fd.h) return;
    const uint32_t idx = y * (uint32_t)fd.w + x;
    const float4 hit = hits[idx];
    const uint32_t tpos = __float_as_uint(hit.w);
    if (tpos == 0xffffffffu) {
        g.prim[idx] = 0xffffffffu;
        g.pos[idx] = make_float4(0.f, 0.f, 0.f, -1.f);
        g.nrm[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
        g.alb[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const V3 ray_dir = v3(q.d[idx]);
    const TriRec T = load_tri_off(sc.tris, tpos << 4);                        // as k_shade
    const MeshDev M = sc.meshes[T.mesh];
    const V3 e1 = v3(T.e1x, T.e1y, T.e1z), e2 = v3(T.e2x, T.e2y, T.e2z);
    const V3 N_0 = normalize(cross(e1, e2));
    const V3 wo = neg(ray_dir);
    const V3 N = N_0 * copysignf(1.0f, dot(wo, N_0));
    const V3 P = v3(fd.eye[0], fd.eye[1], fd.eye[2]) + hit.x * ray_dir;
    V3 albedo = v3(M.material.color);
    if (M.texture_id >= 0 && M.has_texcoord) {
        const float2* tc = sc.tri_tc + (size_t)T.prim * 3;
        const float2 t0 = tc[0], t1 = tc[1], t2 = tc[2];
        const float w0 = 1.f - hit.y - hit.z;
        const float tcx = (w0 * t0.x + hit.y * t1.x) + hit.z * t2.x;
        const float tcy = (w0 * t0.y + hit.y * t1.y) + hit.z * t2.y;
        albedo = v3(tex2d(M.tex, tcx, tcy));
    }
    g.prim[idx] = T.prim;
    g.pos[idx] = f4(P, hit.x);
    g.nrm[idx] = f4(N, 0.f);
    g.alb[idx] = f4(albedo, 0.f);
}

__device__ inline V3 demod(const V3& a)                                    // as the denoiser's
{
    const float s = a.x + a.y + a.z;
    if (s > 0.0f) return v3(fmaxf(a.x, 1.0f / 64.0f), fmaxf(a.y, 1.0f / 64.0f), fmaxf(a.z, 1.0f / 64.0f));
    return v3(1.0f);
}
__device__ inline float edge(float d) { const float t = fmaxf(0.0f, 1.0f - d); return t * t; }
__device__ inline float sq3(const V3& a) { return a.x * a.x + a.y * a.y + a.z * a.z; }

__global__ __launch_bounds__(FOVPT_BLOCK) void k_reconstruct(const FrameDev fd, ReconstructArgs a, const fovpt_float4* __restrict__ in,
                                                             const fovpt_float4* __restrict__ albedo, GBufferDev g,
                                                             fovpt_float4* __restrict__ out_color, uint32_t* __restrict__ out_rgba)
{
    const uint32_t x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= (uint32_t)fd.w || y >= (uint32_t)fd.h) return;
    const uint32_t idx = y * (uint32_t)fd.w + x;
    const fovpt_float4 c = in[idx];
    int wp = 0;
    uint32_t wlx, wly;
    if (find_last_writer(fd, x, y, wp, wlx, wly)) {
        const PassDev& P = fd.pass[wp];
        const int f = P.fill;
        if (f > 1 && (a.levels & (f == 2 ? 1 : 2))) {
            uint32_t ix, iy;
            (void)ring_alive(fd, P, wlx, wly, ix, iy);                      // the anchor: the block's sample pixel (may wrap)
            const float inv_s = a.inv_support[f == 2 ? 0 : 1];
            const bool miss_p = g.prim[idx] == 0xffffffffu;
            const float4 xp4 = g.pos[idx], np4 = g.nrm[idx];
            const V3 Xp = v3(xp4), Np = v3(np4);
            const float tp2 = xp4.w * xp4.w;
            const long long w1 = fd.w - 1, h1 = fd.h - 1;
            float sw = 0.0f;
            V3 acc = v3(0.0f);
#pragma unroll
            for (int j = -1; j <= 1; j++) {
                const long long qy = min(max((long long)iy + (long long)(j * f), 0ll), h1);
                const float hy = fmaxf(0.0f, 1.0f - fabsf((float)((long long)y - qy)) * inv_s);
#pragma unroll
                for (int i = -1; i <= 1; i++) {
                    const long long qx = min(max((long long)ix + (long long)(i * f), 0ll), w1);
                    const float hx = fmaxf(0.0f, 1.0f - fabsf((float)((long long)x - qx)) * inv_s);
                    const uint32_t q = (uint32_t)qy * (uint32_t)fd.w + (uint32_t)qx;
                    const bool miss_q = g.prim[q] == 0xffffffffu;
                    float wn = 1.0f, wz = 1.0f;
                    if (miss_p != miss_q) wn = wz = 0.0f;
                    else if (!miss_p) {
                        const V3 Nq = v3(g.nrm[q]), Xq = v3(g.pos[q]);
                        wn = edge(sq3(Nq - Np) * a.inv_n);
                        const float dz = dot(Np, Xq - Xp);
                        wz = edge(((dz * dz) * a.inv_z) / tp2);
                    }
                    const float wt = ((hx * hy) * wn) * wz;
                    const fovpt_float4 cq = in[q];
                    V3 Iq = v3(cq.x, cq.y, cq.z);
                    if (a.remodulate) {
                        const fovpt_float4 aq = albedo[q];
                        const V3 D = demod(v3(aq.x, aq.y, aq.z));
                        Iq = v3(Iq.x / D.x, Iq.y / D.y, Iq.z / D.z);
                    }
                    sw = sw + wt;
                    acc = acc + Iq * wt;
                }
            }
            if (sw > 0.0f) {
                V3 o = v3(acc.x / sw, acc.y / sw, acc.z / sw);
                if (a.remodulate) o = o * demod(v3(g.alb[idx]));
                out_color[idx] = fovpt_float4{o.x, o.y, o.z, 1.0f};
                out_rgba[idx] = make_color(reinhard(o * 16.0f, 1.0f));
                return;
            }
        }
    }
    out_color[idx] = c;                                                     // unchanged, bit for bit
    out_rgba[idx] = make_color(reinhard(v3(c.x, c.y, c.z) * 16.0f, 1.0f));
}

}  // namespace

void fovpt_launch_gbuffer_rays(hipStream_t st, const FrameDev& fd, RayQueue q, Counters* cnt)
{
    const dim3 grid((fd.w + 63) / 64, (fd.h + 3) / 4);
    hipLaunchKernelGGL(k_gbuffer_rays, grid, dim3(FOVPT_BLOCK), 0, st, fd, q, cnt);
}

void fovpt_launch_gbuffer_fill(hipStream_t st, const FrameDev& fd, SceneView sc, RayQueue q, const float4* hit, GBufferDev g)
{
    const dim3 grid((fd.w + 63) / 64, (fd.h + 3) / 4);
    hipLaunchKernelGGL(k_gbuffer_fill, grid, dim3(FOVPT_BLOCK), 0, st, fd, sc, q, hit, g);
}

void fovpt_launch_reconstruct(hipStream_t st, const FrameDev& fd, const ReconstructArgs& a, const fovpt_float4* in, const fovpt_float4* albedo,
                              GBufferDev g, fovpt_float4* out_color, uint32_t* out_rgba)
{
    const dim3 grid((fd.w + 63) / 64, (fd.h + 3) / 4);
    hipLaunchKernelGGL(k_reconstruct, grid, dim3(FOVPT_BLOCK), 0, st, fd, a, in, albedo, g, out_color, out_rgba);
}
