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
#include "fovpt_post_pixel.h"
#include "fovpt_scene.h"

namespace {

__global__ __launch_bounds__(FOVPT_BLOCK) void k_gbuffer_rays(const FrameDev fd, RayQueue q, Counters* __restrict__ cnt)
{
    uint32_t x, y, idx;
    const bool inside = tile_pixel(fd.w, fd.h, x, y, idx);
    const uint32_t n = (uint32_t)fd.w * (uint32_t)fd.h;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < FOVPT_SHARDS)      // every ray in shard 0 of iteration 0's queue
        cnt->shard[threadIdx.x][FOVPT_CNT_Q(0)] = threadIdx.x == 0 ? n : 0u;
    if (!inside) return;
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
    uint32_t x, y, idx;
    if (!tile_pixel(fd.w, fd.h, x, y, idx)) return;
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

__global__ __launch_bounds__(FOVPT_BLOCK) void k_reconstruct(const FrameDev fd, ReconstructArgs a, const fovpt_float4* __restrict__ in,
                                                             const fovpt_float4* __restrict__ albedo, GBufferDev g,
                                                             fovpt_float4* __restrict__ out_color, uint32_t* __restrict__ out_rgba)
{
    uint32_t x, y, idx;
    if (!tile_pixel(fd.w, fd.h, x, y, idx)) return;
    const fovpt_float4 c = in[idx];
    int wp = 0;
    uint32_t wlx, wly;
    if (find_last_writer(fd, x, y, wp, wlx, wly)) {
        V3 o;
        if (reconstruct_pixel(fd, a, in, albedo, g, GLazy{g, idx}, x, y, idx, wp, wlx, wly, o)) {   // (fovpt_post_pixel.h)
            store_resolved(out_color, out_rgba, idx, o);
            return;
        }
    }
    out_color[idx] = c;                                                     // unchanged, bit for bit
    out_rgba[idx] = resolved_rgba(v3(c));                                   // (c keeps its own w: not store_resolved)
}

}  // namespace

void fovpt_launch_gbuffer_rays(hipStream_t st, const FrameDev& fd, RayQueue q, Counters* cnt)
{
    hipLaunchKernelGGL(k_gbuffer_rays, fovpt_tile_grid(fd.w, fd.h), dim3(FOVPT_BLOCK), 0, st, fd, q, cnt);
}

void fovpt_launch_gbuffer_fill(hipStream_t st, const FrameDev& fd, SceneView sc, RayQueue q, const float4* hit, GBufferDev g)
{
    hipLaunchKernelGGL(k_gbuffer_fill, fovpt_tile_grid(fd.w, fd.h), dim3(FOVPT_BLOCK), 0, st, fd, sc, q, hit, g);
}

void fovpt_launch_reconstruct(hipStream_t st, const FrameDev& fd, const ReconstructArgs& a, const fovpt_float4* in, const fovpt_float4* albedo,
                              GBufferDev g, fovpt_float4* out_color, uint32_t* out_rgba)
{
    hipLaunchKernelGGL(k_reconstruct, fovpt_tile_grid(fd.w, fd.h), dim3(FOVPT_BLOCK), 0, st, fd, a, in, albedo, g, out_color, out_rgba);
}
