// rig.hip -- fovpt_update_animated on the GPU (gfx950): k_rig_pose samples one clip of the rig at the call's time and leaves the
// palettes, rigid matrices and morph weights where refit.hip's skinning, morph and transform kernels read them.
//
// One workgroup, one thread per node.  A thread samples its own node's three channels by binary search over the key times (so
// no sampled pose is staged anywhere), forms the local matrix in registers and waits for its level: the worlds live in LDS
// (FOVPT_RIG_MAX_NODES x 48 B = 48 KiB, static), level l is written between barriers l - 1 and l, and a node reads its parent's
// world from there.  Behind the last barrier the threads stride over the palette entries (W[node] o inverse bind), the rigid
// bindings and the weights.  Every operation is the definition's (include/fovpt.h), unfused (-ffp-contract=off); sine and arc
// cosine are include/fovpt_detmath.h's, whose stated domains (|x| <= 2^20; [-1, 1]) hold [0, pi/2] and [0, 0.9995].
#include "fovpt_device.h"
#include "../../include/fovpt_detmath.h"

namespace {

// Where T falls among a channel's keys: false with k the key to use as given (before the first key, behind the last, STEP);
// true with k the segment's first key and u the place inside it.
__device__ inline bool rig_locate(const RigChannel c, const float* __restrict__ times, float T, uint32_t& k, float& u)
{
    const float* __restrict__ t = times + c.t_first;
    const uint32_t n = c.num_keys;
    u = 0.0f;
    if (T <= t[0]) { k = 0; return false; }
    if (T >= t[n - 1]) { k = n - 1; return false; }
    uint32_t lo = 0, hi = n - 1;                             // t[lo] <= T < t[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (t[mid] <= T) lo = mid; else hi = mid;
    }
    k = lo;
    if (c.interp == FOVPT_RIG_STEP) return false;
    u = (T - t[lo]) / (t[lo + 1] - t[lo]);
    return true;
}

__device__ inline void rig_sample3(const RigDev& r, int32_t ch, float T, float* v)
{
    if (ch < 0) return;                                      // the rest value
    const RigChannel c = r.chan[ch];
    uint32_t k; float u;
    const bool mix = rig_locate(c, r.times, T, k, u);
    const float* __restrict__ a = r.values + c.v_first + 3 * (size_t)k;
    if (!mix) { v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; return; }
#pragma unroll
    for (int e = 0; e < 3; e++) v[e] = a[e] + u * (a[3 + e] - a[e]);
}

__device__ inline void rig_sample4(const RigDev& r, int32_t ch, float T, float* q)
{
    if (ch < 0) return;
    const RigChannel c = r.chan[ch];
    uint32_t k; float u;
    const bool mix = rig_locate(c, r.times, T, k, u);
    const float* __restrict__ p = r.values + c.v_first + 4 * (size_t)k;
    const float ax = p[0], ay = p[1], az = p[2], aw = p[3];
    if (!mix) { q[0] = ax; q[1] = ay; q[2] = az; q[3] = aw; return; }
    float bx = p[4], by = p[5], bz = p[6], bw = p[7];
    float d = ((ax * bx + ay * by) + az * bz) + aw * bw;
    if (d < 0.0f) { bx = -bx; by = -by; bz = -bz; bw = -bw; d = -d; }
    float x, y, z, w;
    if (d > 0.9995f) {
        x = ax + u * (bx - ax); y = ay + u * (by - ay); z = az + u * (bz - az); w = aw + u * (bw - aw);
    } else {
        const float th = fovpt_dm_acosf(d);
        const float s = fovpt_dm_sinf(th);
        const float wa = fovpt_dm_sinf((1.0f - u) * th) / s;
        const float wb = fovpt_dm_sinf(u * th) / s;
        x = wa * ax + wb * bx; y = wa * ay + wb * by; z = wa * az + wb * bz; w = wa * aw + wb * bw;
    }
    const float n = sqrtf(((x * x + y * y) + z * z) + w * w);
    q[0] = x / n; q[1] = y / n; q[2] = z / n; q[3] = w / n;
}

// out = P o L, both row-major 3 x 4
__device__ inline void rig_compose(const float* P, const float* L, float* out)
{
#pragma unroll
    for (int row = 0; row < 3; row++) {
        const float p0 = P[4 * row], p1 = P[4 * row + 1], p2 = P[4 * row + 2], p3 = P[4 * row + 3];
#pragma unroll
        for (int col = 0; col < 3; col++) out[4 * row + col] = (p0 * L[col] + p1 * L[4 + col]) + p2 * L[8 + col];
        out[4 * row + 3] = ((p0 * L[3] + p1 * L[7]) + p2 * L[11]) + p3;
    }
}

__global__ void __launch_bounds__(FOVPT_RIG_MAX_NODES) k_rig_pose(RigDev r, float T)
{
    __shared__ float s_world[FOVPT_RIG_MAX_NODES * 12];
    const uint32_t i = threadIdx.x;
    const bool live = i < r.num_nodes;
    float L[12];
#pragma unroll
    for (int e = 0; e < 12; e++) L[e] = 0.0f;
    uint32_t level = 0;
    int32_t parent = -1;
    if (live) {
        float t[3], q[4], s[3];
        const float* __restrict__ rest = r.rest + 10 * (size_t)i;
        t[0] = rest[0]; t[1] = rest[1]; t[2] = rest[2];
        q[0] = rest[3]; q[1] = rest[4]; q[2] = rest[5]; q[3] = rest[6];
        s[0] = rest[7]; s[1] = rest[8]; s[2] = rest[9];
        rig_sample3(r, r.node_chan[3 * i], T, t);
        rig_sample4(r, r.node_chan[3 * i + 1], T, q);
        rig_sample3(r, r.node_chan[3 * i + 2], T, s);
        const float x = q[0], y = q[1], z = q[2], w = q[3];
        L[0] = (1.0f - 2.0f * (y * y + z * z)) * s[0]; L[1] = (2.0f * (x * y - z * w)) * s[1]; L[2] = (2.0f * (x * z + y * w)) * s[2];
        L[4] = (2.0f * (x * y + z * w)) * s[0]; L[5] = (1.0f - 2.0f * (x * x + z * z)) * s[1]; L[6] = (2.0f * (y * z - x * w)) * s[2];
        L[8] = (2.0f * (x * z - y * w)) * s[0]; L[9] = (2.0f * (y * z + x * w)) * s[1]; L[10] = (1.0f - 2.0f * (x * x + y * y)) * s[2];
        L[3] = t[0]; L[7] = t[1]; L[11] = t[2];
        level = r.level[i];
        parent = r.parent[i];
    }
    // a level per barrier: a node's parent is one level up, written before the barrier this node's level waits behind
    for (uint32_t lv = 0; lv < r.num_levels; lv++) {
        if (live && level == lv) {
            float W[12];
            if (parent < 0) {
#pragma unroll
                for (int e = 0; e < 12; e++) W[e] = L[e];
            } else {
                float P[12];
#pragma unroll
                for (int e = 0; e < 12; e++) P[e] = s_world[12 * parent + e];
                rig_compose(P, L, W);
            }
#pragma unroll
            for (int e = 0; e < 12; e++) s_world[12 * i + e] = W[e];
        }
        __syncthreads();
    }
    for (uint32_t e = threadIdx.x; e < 12 * r.num_nodes; e += blockDim.x) r.world[e] = s_world[e];
    for (uint32_t j = threadIdx.x; j < r.num_pal; j += blockDim.x) {
        float P[12], B[12], J[12];
        const uint32_t node = r.pal_node[j];
#pragma unroll
        for (int e = 0; e < 12; e++) { P[e] = s_world[12 * node + e]; B[e] = r.inv_bind[12 * (size_t)j + e]; }
        rig_compose(P, B, J);
        float* __restrict__ dst = r.skin_pal + 12 * (size_t)r.pal_dst[j];
#pragma unroll
        for (int e = 0; e < 12; e++) { dst[e] = J[e]; r.palette[12 * (size_t)j + e] = J[e]; }
    }
    for (uint32_t j = threadIdx.x; j < r.num_rigid; j += blockDim.x) {
        const uint32_t node = r.rigid_node[j];
#pragma unroll
        for (int e = 0; e < 12; e++) r.rigid[12 * (size_t)j + e] = s_world[12 * node + e];
    }
    // the weights: per bound morphed mesh its channel's keys are rows of num_targets floats
    for (uint32_t j = 0; j < r.num_wjobs; j++) {
        const RigWeights job = r.wjobs[j];
        const int32_t ch = r.w_chan[j];
        float* __restrict__ dst = r.morph_w + job.w_first;
        if (ch < 0) {
            for (uint32_t t = threadIdx.x; t < job.num_targets; t += blockDim.x) dst[t] = 0.0f;
            continue;
        }
        const RigChannel c = r.chan[ch];
        uint32_t k; float u;
        const bool mix = rig_locate(c, r.times, T, k, u);
        const float* __restrict__ a = r.values + c.v_first + (size_t)job.num_targets * k;
        const float* __restrict__ b = a + job.num_targets;
        for (uint32_t t = threadIdx.x; t < job.num_targets; t += blockDim.x) dst[t] = mix ? a[t] + u * (b[t] - a[t]) : a[t];
    }
}

}  // namespace

void fovpt_launch_rig_pose(hipStream_t st, const RigDev& r, float time, uint32_t threads)
{
    hipLaunchKernelGGL(k_rig_pose, dim3(1), dim3(threads), 0, st, r, time);
}
