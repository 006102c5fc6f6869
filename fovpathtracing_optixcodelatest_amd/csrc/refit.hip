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
//
// Also here: fovpt_update_transforms' k_transform_vertices (rest positions through per-mesh 3 x 4 matrices into the vertex array,
// ahead of the same refit; k_transform_vertices_dev: the same for fovpt_update_animated's rigid bindings), fovpt_update_skinned's k_skin_vertices (the same with a matrix blended per vertex from its mesh's joint
// palette), fovpt_update_morphed's k_morph_vertices / k_morph_skin_vertices (the rest positions plus their weighted morph deltas,
// the second then through the skin) and fovpt_hierarchy_cost's k_tree_cost / k_tree_cost_final (the SAH cost of the nodes in
// binary64).
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

// fovpt_update_transforms: the y grid dimension runs over the batch's meshes, x strides over a mesh's vertices.  Each vertex of
// rest goes through its mesh's matrix into vtx: three dependent unfused operations per row (-ffp-contract=off), 24 B of traffic.
__global__ void k_transform_vertices(VertexTransform g, const float* __restrict__ rest, float* __restrict__ vtx)
{
    for (int u = blockIdx.y; u < g.count; u += gridDim.y) {
        const float* m = g.m[u];
        const float* __restrict__ src = rest + 3 * (size_t)g.first[u];
        float* __restrict__ dst = vtx + 3 * (size_t)g.first[u];
        const size_t n = g.n[u];
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
            const float x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
            dst[3 * i] = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
            dst[3 * i + 1] = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
            dst[3 * i + 2] = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
        }
    }
}

// fovpt_update_animated's rigid bindings: k_transform_vertices with each mesh's matrix read from device memory (k_rig_pose wrote
// it earlier on the stream); the arithmetic is the same expression.
__global__ void k_transform_vertices_dev(VertexTransformDev g, const float* __restrict__ rest, float* __restrict__ vtx)
{
    for (int u = blockIdx.y; u < g.count; u += gridDim.y) {
        const float* __restrict__ gm = g.m[u];
        float m[12];
#pragma unroll
        for (int e = 0; e < 12; e++) m[e] = gm[e];
        const float* __restrict__ src = rest + 3 * (size_t)g.first[u];
        float* __restrict__ dst = vtx + 3 * (size_t)g.first[u];
        const size_t n = g.n[u];
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
            const float x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
            dst[3 * i] = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
            dst[3 * i + 1] = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
            dst[3 * i + 2] = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
        }
    }
}

// fovpt_update_skinned: k_transform_vertices' launch shape.  Per vertex 12 B of rest, one 8-byte load of the four joint indices,
// one 16-byte load of the weights and four 48-byte palette rows (at most 48 KB per mesh, read by every block of the mesh: cache
// resident after the first touch); the blended matrix entry by entry, then the vertex through it, every operation unfused
// (-ffp-contract=off); 12 B written.  Joint indices were checked against the palette's size by fovpt_set_skins.
__global__ void k_skin_vertices(VertexSkin g, const float* __restrict__ rest, const uint2* __restrict__ joints, const float4* __restrict__ weights,
                                float* __restrict__ vtx)
{
    for (int u = blockIdx.y; u < g.count; u += gridDim.y) {
        const float* __restrict__ pal = g.pal[u];
        const float* __restrict__ src = rest + 3 * (size_t)g.first[u];
        float* __restrict__ dst = vtx + 3 * (size_t)g.first[u];
        const uint2* __restrict__ jv = joints + g.skin[u];
        const float4* __restrict__ wv = weights + g.skin[u];
        const size_t n = g.n[u];
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
            const uint2 j = jv[i];
            const float4 w = wv[i];
            const float x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
            const float* __restrict__ j0 = pal + 12 * (j.x & 0xffffu);
            const float* __restrict__ j1 = pal + 12 * (j.x >> 16);
            const float* __restrict__ j2 = pal + 12 * (j.y & 0xffffu);
            const float* __restrict__ j3 = pal + 12 * (j.y >> 16);
            float m[12];
#pragma unroll
            for (int e = 0; e < 12; e++) m[e] = ((w.x * j0[e] + w.y * j1[e]) + w.z * j2[e]) + w.w * j3[e];
            dst[3 * i] = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
            dst[3 * i + 1] = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
            dst[3 * i + 2] = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
        }
    }
}

// fovpt_update_morphed: k_skin_vertices' launch shape.  Per vertex 12 B of rest and its two offsets into the entries; per entry
// the record's target word, that target's weight (at most 1 KB per mesh, read by every thread: cache resident), and only where
// the weight is not zero the 16-byte record itself: p = p + w * d per coordinate in ascending targets, every operation unfused
// (-ffp-contract=off); a vertex none of whose targets is active is stored as it was loaded, -0 included.  With SKIN the morphed
// position goes through k_skin_vertices' blend (restated here: that kernel stays as it is) instead of to memory; 12 B written.
// Offsets, targets and joint indices were laid out or checked by fovpt_set_morphs / fovpt_set_skins.
template <bool SKIN>
__device__ inline void morph_vertices(const VertexMorph& g, const float* __restrict__ rest, const uint32_t* __restrict__ off,
                                      const MorphEntry* __restrict__ ent, const uint2* __restrict__ joints, const float4* __restrict__ weights,
                                      float* __restrict__ vtx)
{
    for (int u = blockIdx.y; u < g.count; u += gridDim.y) {
        const float* __restrict__ mw = g.w[u];
        const float* __restrict__ src = rest + 3 * (size_t)g.first[u];
        float* __restrict__ dst = vtx + 3 * (size_t)g.first[u];
        const uint32_t* __restrict__ ov = off + g.off[u];
        const size_t n = g.n[u];
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
            float x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
            const uint32_t end = ov[i + 1];
            for (uint32_t k = ov[i]; k < end; k++) {
                const float t = mw[ent[k].target];
                if (t != 0.0f) {                                          // +0 and -0 skip the entry: its record is not fetched
                    const float4 d = reinterpret_cast<const float4*>(ent)[k];
                    x = x + t * d.x; y = y + t * d.y; z = z + t * d.z;
                }
            }
            if constexpr (SKIN) {
                const float* __restrict__ pal = g.pal[u];
                const uint2 j = joints[g.skin[u] + i];
                const float4 w = weights[g.skin[u] + i];
                const float* __restrict__ j0 = pal + 12 * (j.x & 0xffffu);
                const float* __restrict__ j1 = pal + 12 * (j.x >> 16);
                const float* __restrict__ j2 = pal + 12 * (j.y & 0xffffu);
                const float* __restrict__ j3 = pal + 12 * (j.y >> 16);
                float m[12];
#pragma unroll
                for (int e = 0; e < 12; e++) m[e] = ((w.x * j0[e] + w.y * j1[e]) + w.z * j2[e]) + w.w * j3[e];
                dst[3 * i] = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
                dst[3 * i + 1] = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
                dst[3 * i + 2] = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
            } else {
                dst[3 * i] = x; dst[3 * i + 1] = y; dst[3 * i + 2] = z;
            }
        }
    }
}

__global__ void k_morph_vertices(VertexMorph g, const float* __restrict__ rest, const uint32_t* __restrict__ off, const MorphEntry* __restrict__ ent,
                                 float* __restrict__ vtx)
{
    morph_vertices<false>(g, rest, off, ent, nullptr, nullptr, vtx);
}

__global__ void k_morph_skin_vertices(VertexMorph g, const float* __restrict__ rest, const uint32_t* __restrict__ off, const MorphEntry* __restrict__ ent,
                                      const uint2* __restrict__ joints, const float4* __restrict__ weights, float* __restrict__ vtx)
{
    morph_vertices<true>(g, rest, off, ent, joints, weights, vtx);
}

// fovpt_hierarchy_cost: dx dy + dy dz + dz dx of a box in binary64
__device__ inline double box_area(double dx, double dy, double dz) { return dx * dy + dy * dz + dz * dx; }

// sums s[0 .. FOVPT_BLOCK) into s[0] in a fixed order (every thread of the block calls it)
__device__ inline void block_sum(double* s)
{
    __syncthreads();
    for (uint32_t w = FOVPT_BLOCK / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
}

// One thread per (node, child slot): the area of a live entry, as a node entry's or a leaf entry's; the block's two sums go to
// partial[2 b], partial[2 b + 1].  No atomics: the order of every addition is fixed by the indices alone.
__global__ void __launch_bounds__(FOVPT_BLOCK) k_tree_cost(const BvhNode4* __restrict__ nodes, uint32_t num_nodes, double* __restrict__ partial)
{
    __shared__ double s_node[FOVPT_BLOCK], s_leaf[FOVPT_BLOCK];
    const uint64_t t = (uint64_t)blockIdx.x * FOVPT_BLOCK + threadIdx.x;
    double a_node = 0.0, a_leaf = 0.0;
    if (t < 4ull * num_nodes) {
        const float4* rec = reinterpret_cast<const float4*>(&nodes[t >> 2].c[t & 3u]);
        const float4 r0 = rec[0], r1 = rec[1];             // {lo.xyz, hi.x}, {hi.yz, code, rank}
        if (r0.x < INFINITY) {
            const double a = box_area((double)r0.w - (double)r0.x, (double)r1.x - (double)r0.y, (double)r1.y - (double)r0.z);
            if (__float_as_int(r1.z) >= 0) a_node = a; else a_leaf = a;
        }
    }
    s_node[threadIdx.x] = a_node; s_leaf[threadIdx.x] = a_leaf;
    block_sum(s_node);
    block_sum(s_leaf);
    if (threadIdx.x == 0) { partial[2 * (size_t)blockIdx.x] = s_node[0]; partial[2 * (size_t)blockIdx.x + 1] = s_leaf[0]; }
}

// One block: thread k sums the partials k, k + FOVPT_BLOCK, ... in index order, the block sums those; thread 0 adds the area of
// the union of the root's live entries and writes the record.
__global__ void __launch_bounds__(FOVPT_BLOCK) k_tree_cost_final(const BvhNode4* __restrict__ nodes, const double* __restrict__ partial, uint32_t nblocks,
                                                                 TreeCostRecord* __restrict__ out)
{
    __shared__ double s_node[FOVPT_BLOCK], s_leaf[FOVPT_BLOCK];
    double a_node = 0.0, a_leaf = 0.0;
    for (uint32_t b = threadIdx.x; b < nblocks; b += FOVPT_BLOCK) { a_node += partial[2 * (size_t)b]; a_leaf += partial[2 * (size_t)b + 1]; }
    s_node[threadIdx.x] = a_node; s_leaf[threadIdx.x] = a_leaf;
    block_sum(s_node);
    block_sum(s_leaf);
    if (threadIdx.x != 0) return;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < 4; k++) {
        const BvhChild c = nodes[0].c[k];
        if (!(c.lox < INFINITY)) continue;
        lo[0] = fminf(lo[0], c.lox); lo[1] = fminf(lo[1], c.loy); lo[2] = fminf(lo[2], c.loz);
        hi[0] = fmaxf(hi[0], c.hix); hi[1] = fmaxf(hi[1], c.hiy); hi[2] = fmaxf(hi[2], c.hiz);
    }
    TreeCostRecord r;
    r.root = box_area((double)hi[0] - (double)lo[0], (double)hi[1] - (double)lo[1], (double)hi[2] - (double)lo[2]);
    r.node = s_node[0]; r.leaf = s_leaf[0];
    r.cost = (r.root + r.node + 2.7 * r.leaf) / r.root;
    *out = r;
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

void fovpt_launch_transform_vertices(hipStream_t st, const VertexTransform& g, const float* rest, float* vtx)
{
    if (g.count <= 0 || g.max_n == 0) return;
    const uint64_t n = g.max_n;
    const uint32_t gx = (uint32_t)(n < 1024ull * FOVPT_BLOCK ? (n + FOVPT_BLOCK - 1) / FOVPT_BLOCK : 1024ull);
    hipLaunchKernelGGL(k_transform_vertices, dim3(gx, (uint32_t)g.count), dim3(FOVPT_BLOCK), 0, st, g, rest, vtx);
}

void fovpt_launch_transform_vertices_dev(hipStream_t st, const VertexTransformDev& g, const float* rest, float* vtx)
{
    if (g.count <= 0 || g.max_n == 0) return;
    const uint64_t n = g.max_n;
    const uint32_t gx = (uint32_t)(n < 1024ull * FOVPT_BLOCK ? (n + FOVPT_BLOCK - 1) / FOVPT_BLOCK : 1024ull);
    hipLaunchKernelGGL(k_transform_vertices_dev, dim3(gx, (uint32_t)g.count), dim3(FOVPT_BLOCK), 0, st, g, rest, vtx);
}

void fovpt_launch_skin_vertices(hipStream_t st, const VertexSkin& g, const float* rest, const uint2* joints, const float4* weights, float* vtx)
{
    if (g.count <= 0 || g.max_n == 0) return;
    const uint64_t n = g.max_n;
    const uint32_t gx = (uint32_t)(n < 1024ull * FOVPT_BLOCK ? (n + FOVPT_BLOCK - 1) / FOVPT_BLOCK : 1024ull);
    hipLaunchKernelGGL(k_skin_vertices, dim3(gx, (uint32_t)g.count), dim3(FOVPT_BLOCK), 0, st, g, rest, joints, weights, vtx);
}

void fovpt_launch_morph_vertices(hipStream_t st, const VertexMorph& g, const float* rest, const uint32_t* off, const MorphEntry* ent, float* vtx)
{
    if (g.count <= 0 || g.max_n == 0) return;
    const uint64_t n = g.max_n;
    const uint32_t gx = (uint32_t)(n < 1024ull * FOVPT_BLOCK ? (n + FOVPT_BLOCK - 1) / FOVPT_BLOCK : 1024ull);
    hipLaunchKernelGGL(k_morph_vertices, dim3(gx, (uint32_t)g.count), dim3(FOVPT_BLOCK), 0, st, g, rest, off, ent, vtx);
}

void fovpt_launch_morph_skin_vertices(hipStream_t st, const VertexMorph& g, const float* rest, const uint32_t* off, const MorphEntry* ent,
                                      const uint2* joints, const float4* weights, float* vtx)
{
    if (g.count <= 0 || g.max_n == 0) return;
    const uint64_t n = g.max_n;
    const uint32_t gx = (uint32_t)(n < 1024ull * FOVPT_BLOCK ? (n + FOVPT_BLOCK - 1) / FOVPT_BLOCK : 1024ull);
    hipLaunchKernelGGL(k_morph_skin_vertices, dim3(gx, (uint32_t)g.count), dim3(FOVPT_BLOCK), 0, st, g, rest, off, ent, joints, weights, vtx);
}

void fovpt_launch_tree_cost(hipStream_t st, const BvhNode4* nodes, uint32_t num_nodes, double* partial, TreeCostRecord* rec)
{
    const uint32_t nblocks = fovpt_tree_cost_blocks(num_nodes);
    if (nblocks) hipLaunchKernelGGL(k_tree_cost, dim3(nblocks), dim3(FOVPT_BLOCK), 0, st, nodes, num_nodes, partial);
    hipLaunchKernelGGL(k_tree_cost_final, dim3(1), dim3(FOVPT_BLOCK), 0, st, nodes, partial, nblocks, rec);
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
