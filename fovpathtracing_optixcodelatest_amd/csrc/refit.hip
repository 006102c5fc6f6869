// refit.hip -- fovpt_update_vertices on the GPU (gfx950): new vertex positions into the scene's vertex array, then a refit of
// the wide hierarchy over them.
//
// The tree keeps its shape.  One launch per level of the wide tree, deepest first, one thread per (node, child slot): a leaf
// child rewrites its triangle records from the vertices (v0, e1 = v1 - v0, e2 = v2 - v0 exactly as the build emits them) and
// takes the union of their padded boxes (fovpt_tri_pad, the build's expression); a node child takes the union of that node's
// non-empty child boxes, written by the previous launch -- the kernel boundary is the only hand-off between threads, so
// nothing is shared inside a launch and no fence or atomic is needed.  An empty slot (lo = hi = +inf) is left as it is: a
// union over it would make the parent's box infinite.  min / max are exact, so a refit over unchanged vertices reproduces the
// build's boxes bit for bit (without spatial splits: a split reference's clipped box becomes its whole triangle's box).
#include "fovpt_device.h"

namespace {

// the padded box of the triangle p[0..8], as the build's k_tri_bounds computes it
__device__ inline void tri_box(const float* p, float* lo, float* hi)
{
    float ext = 0.f, mag = 0.f;
    for (int a = 0; a < 3; a++) {
        const float x0 = p[a], x1 = p[3 + a], x2 = p[6 + a];
        lo[a] = fminf(x0, fminf(x1, x2)); hi[a] = fmaxf(x0, fmaxf(x1, x2));
        ext = fmaxf(ext, hi[a] - lo[a]);
        mag = fmaxf(mag, fmaxf(fabsf(lo[a]), fabsf(hi[a])));
    }
    const float pad = fovpt_tri_pad(ext, mag);
    for (int a = 0; a < 3; a++) { lo[a] -= pad; hi[a] += pad; }
}

__global__ void k_gather_vertices(VertexGather g, float* __restrict__ vtx)
{
    for (int u = blockIdx.y; u < g.count; u += gridDim.y) {
        const float* __restrict__ src = g.src[u];
        float* __restrict__ dst = vtx + 3 * (size_t)g.dst[u];
        const size_t n = 3 * (size_t)g.n[u];
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
    }
}

// fovpt_temporal_motion's tracking: the positions a mesh has now into vtx_prev, before this update overwrites them, and the
// mesh's mark (one plain vector store)
__global__ void k_gather_vertices_prev(VertexTrack g, const float* __restrict__ vtx, float* __restrict__ vtx_prev, uint64_t* __restrict__ mark,
                                       uint64_t epoch)
{
    for (int u = blockIdx.y; u < g.count; u += gridDim.y) {
        const size_t first = 3 * (size_t)g.first[u], n = 3 * (size_t)g.n[u];
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) vtx_prev[first + i] = vtx[first + i];
        if (blockIdx.x == 0 && threadIdx.x == 0) mark[g.mesh[u]] = epoch;
    }
}

__global__ void k_refit_level(uint32_t first, uint32_t count, BvhNode4* __restrict__ nodes, TriRec* __restrict__ tris,
                              const uint3* __restrict__ tri_vidx, const float* __restrict__ vtx)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 4u * count) return;
    float4* rec = reinterpret_cast<float4*>(&nodes[first + (t >> 2)].c[t & 3u]);
    const float4 r0 = rec[0], r1 = rec[1];                 // {lo.xyz, hi.x}, {hi.yz, code, rank}
    if (!(r0.x < INFINITY)) return;                        // empty slot
    const int32_t code = __float_as_int(r1.z);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (code < 0) {
        const uint32_t lcode = (uint32_t)~code, n = (lcode & 7u) + 1u, t0 = (lcode >> 3) / 3u;
        for (uint32_t j = 0; j < n; j++) {
            float4* tr = reinterpret_cast<float4*>(&tris[t0 + j]);
            const float4 w2 = tr[2];                       // {e2z, prim, mesh, pad}
            const uint3 iv = tri_vidx[__float_as_uint(w2.y)];
            const uint32_t vi[3] = {iv.x, iv.y, iv.z};
            float p[9];
            for (int v = 0; v < 3; v++)
                for (int a = 0; a < 3; a++) p[3 * v + a] = vtx[3 * (size_t)vi[v] + a];
            // k_emit_tris_generic's record
            tr[0] = make_float4(p[0], p[1], p[2], p[3] - p[0]);
            tr[1] = make_float4(p[4] - p[1], p[5] - p[2], p[6] - p[0], p[7] - p[1]);
            tr[2] = make_float4(p[8] - p[2], w2.y, w2.z, w2.w);
            float blo[3], bhi[3];
            tri_box(p, blo, bhi);
            for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], blo[a]); hi[a] = fmaxf(hi[a], bhi[a]); }
        }
    } else {
        const float4* ch = reinterpret_cast<const float4*>(&nodes[code]);
        for (int k = 0; k < 4; k++) {
            const float4 c0 = ch[2 * k], c1 = ch[2 * k + 1];
            if (!(c0.x < INFINITY)) continue;              // the child's empty slots
            lo[0] = fminf(lo[0], c0.x); lo[1] = fminf(lo[1], c0.y); lo[2] = fminf(lo[2], c0.z);
            hi[0] = fmaxf(hi[0], c0.w); hi[1] = fmaxf(hi[1], c1.x); hi[2] = fmaxf(hi[2], c1.y);
        }
    }
    rec[0] = make_float4(lo[0], lo[1], lo[2], hi[0]);
    rec[1] = make_float4(hi[1], hi[2], r1.z, r1.w);
}

__global__ void k_flatten(uint32_t n, const uint3* __restrict__ tri_vidx, const float* __restrict__ vtx, float* __restrict__ flat)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint3 iv = tri_vidx[i];
    const uint32_t vi[3] = {iv.x, iv.y, iv.z};
    for (int v = 0; v < 3; v++)
        for (int a = 0; a < 3; a++) flat[9 * (size_t)i + 3 * v + a] = vtx[3 * (size_t)vi[v] + a];
}

}  // namespace

void fovpt_launch_gather_vertices(hipStream_t st, const VertexGather& g, float* vtx)
{
    if (g.count <= 0 || g.max_n == 0) return;
    const uint64_t floats = 3ull * g.max_n;
    const uint32_t gx = (uint32_t)(floats < 1024ull * FOVPT_BLOCK ? (floats + FOVPT_BLOCK - 1) / FOVPT_BLOCK : 1024ull);
    hipLaunchKernelGGL(k_gather_vertices, dim3(gx, (uint32_t)g.count), dim3(FOVPT_BLOCK), 0, st, g, vtx);
}

void fovpt_launch_gather_vertices_prev(hipStream_t st, const VertexTrack& g, const float* vtx, float* vtx_prev, uint64_t* mark, uint64_t epoch)
{
    if (g.count <= 0) return;
    const uint64_t floats = 3ull * (g.max_n ? g.max_n : 1u);                  // (a mesh without vertices still gets its mark)
    const uint32_t gx = (uint32_t)(floats < 1024ull * FOVPT_BLOCK ? (floats + FOVPT_BLOCK - 1) / FOVPT_BLOCK : 1024ull);
    hipLaunchKernelGGL(k_gather_vertices_prev, dim3(gx, (uint32_t)g.count), dim3(FOVPT_BLOCK), 0, st, g, vtx, vtx_prev, mark, epoch);
}

void fovpt_launch_refit(hipStream_t st, BvhNode4* nodes, TriRec* tris, const uint32_t* levels, uint32_t num_levels, const uint3* tri_vidx,
                        const float* vtx)
{
    for (uint32_t L = num_levels; L-- > 0;) {
        const uint32_t first = levels[L], count = levels[L + 1] - first;
        if (count) hipLaunchKernelGGL(k_refit_level, dim3((4u * count + FOVPT_BLOCK - 1) / FOVPT_BLOCK), dim3(FOVPT_BLOCK), 0, st, first, count,
                                      nodes, tris, tri_vidx, vtx);
    }
}

void fovpt_launch_flatten(hipStream_t st, uint32_t n, const uint3* tri_vidx, const float* vtx, float* flat)
{
    if (n) hipLaunchKernelGGL(k_flatten, dim3((n + FOVPT_BLOCK - 1) / FOVPT_BLOCK), dim3(FOVPT_BLOCK), 0, st, n, tri_vidx, vtx, flat);
}
