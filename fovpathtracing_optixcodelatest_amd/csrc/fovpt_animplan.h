// fovpt_animplan.h -- what fovpt_set_skins, fovpt_set_morphs and fovpt_set_rig accept and how they lay their data out, and the overflow
// rules of the fovpt_update_* calls, as plain host C++17: no HIP, no fovpt_ctx, so that g++ compiles it alone and
// tests/cpp/anim_plan_test.cpp runs it under the address and undefined-behaviour sanitizers.  api_animate.hip gives a plan function
// an AnimScene (what the rules need of the scene and of the skins and morphs it has now) and the caller's description, and gets
// back a plan: refused, with FOVPT_E_INVALID and the text fovpt_last_error returns, or accepted, with every table the entry point
// uploads and keeps.  The order of the checks is part of the contract: it decides which text a caller sees and how much of the
// caller's memory is read before a refusal.  This header is the definition of the rules and of the layouts.
#pragma once

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fovpt.h"

// What the host lays out and the kernels read (rig.hip, refit.hip)
struct RigChannel { uint32_t t_first, v_first, num_keys, interp; };      // its keys' places in times / values
struct RigWeights { uint32_t w_first, num_targets; };                   // a bound morphed mesh's place in morph_w
struct MorphEntry { float dx, dy, dz; uint32_t target; };               // 16 bytes
// A binding of the rig, in the description's order: what its mesh goes through and its place among the rigid matrices
struct RigBound { int32_t mesh; uint32_t rigid; bool skinned, morphed, is_rigid; };

// What the rules read of one mesh: its vertex count, the skin it has now (joints 0: none; its first joint in skin_pal) and the morph
// targets it has now (targets 0: none; its entries and its first weight in morph_w)
struct AnimMesh { uint32_t nv = 0, skin_joints = 0, pal_first = 0, morph_targets = 0, w_first = 0; size_t morph_entries = 0; };
struct AnimScene { std::vector<AnimMesh> mesh; };

// Every plan and every overflow check: accepted (code FOVPT_OK) or refused.  refuse(): the text as fail() formats it.
struct AnimVerdict {
    int code = FOVPT_OK;
    std::string text;
    __attribute__((format(printf, 2, 3))) int refuse(const char* fmt, ...)
    {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        text = buf;
        return code = FOVPT_E_INVALID;
    }
};

// A mesh named by a list: it exists and no earlier entry named it (seen: one flag per mesh)
inline int anim_list_mesh(AnimVerdict& V, std::vector<char>& seen, const char* who, int m)
{
    const int nmesh = (int)seen.size();
    if (m < 0 || m >= nmesh) return V.refuse("%s: mesh %d of %d", who, m, nmesh);
    if (seen[m]) return V.refuse("%s: mesh %d is listed twice", who, m);
    seen[m] = 1;
    return FOVPT_OK;
}

// ---- the overflow rules of the fovpt_update_* calls: every intermediate value of the kernels' expressions stays finite ----------
// fovpt_update_transforms: one 3 x 4 matrix over positions within A (one matrix is not blended: no second part)
inline int anim_check_transform(AnimVerdict& V, const char* who, int mesh, const float* m, double A)
{
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(m[i])) return V.refuse("%s: mesh %d matrix entry %d is not finite", who, mesh, i);
    for (int r = 0; r < 3; r++) {
        const float* row = m + 4 * r;
        const double bound = (std::fabs((double)row[0]) + std::fabs((double)row[1]) + std::fabs((double)row[2])) * A + std::fabs((double)row[3]);
        if (bound > 0x1p127) return V.refuse("%s: mesh %d row %d could overflow (bound %g > 2^127)", who, mesh, r, bound);
    }
    return FOVPT_OK;
}

// A host palette (fovpt_update_skinned, fovpt_update_morphed): S the skin's largest weight sum, B a bound of the |coordinates| that go
// through the matrices
inline int anim_check_palette(AnimVerdict& V, const char* who, int mesh, const float* matrices, uint32_t num_joints, double S, double B)
{
    for (size_t i = 0; i < 12 * (size_t)num_joints; i++)
        if (!std::isfinite(matrices[i])) return V.refuse("%s: mesh %d joint %zu entry %zu is not finite", who, mesh, i / 12, i % 12);
    for (size_t r = 0; r < 3 * (size_t)num_joints; r++) {
        const float* row = matrices + 4 * r;
        const double bound = S * ((std::fabs((double)row[0]) + std::fabs((double)row[1]) + std::fabs((double)row[2])) * B + std::fabs((double)row[3]));
        if (bound > 0x1p127) return V.refuse("%s: mesh %d joint %zu row %zu could overflow (bound %g > 2^127)", who, mesh, r / 3, r % 3, bound);
        // (the blended matrix is formed first: its entries are within S times the palette's, which the row's bound covers
        // for the fourth column and, for the others, only when B >= 1)
        const double entry = S * std::fmax(std::fmax(std::fabs((double)row[0]), std::fabs((double)row[1])), std::fabs((double)row[2]));
        if (entry > 0x1p127) return V.refuse("%s: mesh %d joint %zu row %zu: a blended entry could overflow (%g > 2^127)", who, mesh, r / 3, r % 3, entry);
    }
    return FOVPT_OK;
}

// Host morph weights over rest positions within A, D[t] the largest |delta component| of target t.  *B: the morphed positions' bound,
// what a palette on the same pose is checked with.
inline int anim_check_weights(AnimVerdict& V, const char* who, int mesh, const float* weights, uint32_t num_targets, const double* D, double A, double* B)
{
    *B = A;
    for (uint32_t t = 0; t < num_targets; t++) {
        if (!std::isfinite(weights[t])) return V.refuse("%s: mesh %d: weight %u is not finite", who, mesh, t);
        *B += std::fabs((double)weights[t]) * D[t];
    }
    if (*B > 0x1p127) return V.refuse("%s: mesh %d could overflow (bound %g > 2^127)", who, mesh, *B);
    return FOVPT_OK;
}

// ---- fovpt_set_skins ------------------------------------------------------------------------------------------------------
// Every call lays the device copies out anew: the skinned meshes' vertices (skin_joints, skin_weights) and joints (skin_pal) in mesh
// order.
struct SkinPlan : AnimVerdict {
    std::vector<double> S;                                    // per listed skin: its largest four-weight sum, in binary64
    std::vector<uint32_t> num_joints, first, pal_first;       // per mesh: the joints it has after the call, its first vertex and joint
    size_t verts = 0, joints = 0;                             // of the skinned meshes
    size_t joints_bytes = 0, weights_bytes = 0, pal_bytes = 0;        // the device buffers (0: none)
};

inline int plan_skins(const AnimScene& sc, const char* who, const fovpt_mesh_skin* skins, int num, SkinPlan& P)
{
    const int nmesh = (int)sc.mesh.size();
    std::vector<char> seen((size_t)nmesh, 0);
    P.S.assign((size_t)(num > 0 ? num : 0), 0.0);
    for (int k = 0; k < num; k++) {
        const fovpt_mesh_skin& K = skins[k];
        if (anim_list_mesh(P, seen, who, K.mesh)) return P.code;
        if (K._reserved) return P.refuse("%s: mesh %d: _reserved is %u", who, K.mesh, K._reserved);
        if (K.num_vertices != sc.mesh[K.mesh].nv)
            return P.refuse("%s: mesh %d has %u vertices, not %u", who, K.mesh, sc.mesh[K.mesh].nv, K.num_vertices);
        if (K.num_joints > FOVPT_SKIN_MAX_JOINTS) return P.refuse("%s: mesh %d: %u joints (at most %d)", who, K.mesh, K.num_joints, FOVPT_SKIN_MAX_JOINTS);
        if (K.num_joints == 0) {
            if (K.joints || K.weights) return P.refuse("%s: mesh %d: no joints, but a pointer (removing a skin takes two null pointers)", who, K.mesh);
            continue;
        }
        if (!K.joints || !K.weights) return P.refuse("%s: mesh %d: null joints or weights", who, K.mesh);
        for (size_t i = 0; i < 4 * (size_t)K.num_vertices; i++) {
            if (K.joints[i] >= K.num_joints) return P.refuse("%s: mesh %d vertex %zu: joint %u of %u", who, K.mesh, i / 4, (unsigned)K.joints[i], K.num_joints);
            if (!(K.weights[i] >= 0.0f && K.weights[i] <= 1.0f)) return P.refuse("%s: mesh %d vertex %zu: weight %g is not in [0, 1]", who, K.mesh, i / 4, (double)K.weights[i]);
        }
        for (size_t i = 0; i < (size_t)K.num_vertices; i++) {
            const float* w = K.weights + 4 * i;
            P.S[k] = std::fmax(P.S[k], (((double)w[0] + (double)w[1]) + (double)w[2]) + (double)w[3]);
        }
    }
    // the new layout
    P.num_joints.assign((size_t)nmesh, 0);
    for (int m = 0; m < nmesh; m++) P.num_joints[m] = sc.mesh[m].skin_joints;
    for (int k = 0; k < num; k++) P.num_joints[skins[k].mesh] = skins[k].num_joints;
    for (int m = 0; m < nmesh; m++)
        if (P.num_joints[m]) { P.verts += sc.mesh[m].nv; P.joints += P.num_joints[m]; }
    if (P.verts >= (1ull << 32)) return P.refuse("%s: more than 2^32 - 1 skinned vertices", who);
    P.first.assign((size_t)nmesh, 0); P.pal_first.assign((size_t)nmesh, 0);
    uint32_t first = 0, pal_first = 0;
    for (int m = 0; m < nmesh; m++) {
        P.first[m] = first; P.pal_first[m] = pal_first;
        if (!P.num_joints[m]) continue;
        first += sc.mesh[m].nv; pal_first += P.num_joints[m];
    }
    if (P.joints) { P.joints_bytes = P.verts ? P.verts * 8 : 8; P.weights_bytes = P.verts ? P.verts * 16 : 16; P.pal_bytes = P.joints * 48; }
    return FOVPT_OK;
}

// ---- fovpt_set_morphs -----------------------------------------------------------------------------------------------------
// A mesh's targets are kept transposed into a per-vertex list of {delta, target} records sorted by target (what the kernel walks:
// the order of the definition is the order in memory).  Every call lays the device copies out anew: the morphed meshes' offsets
// (morph_off: num_vertices + 1 each, absolute into morph_ent), entries (morph_ent) and weights (morph_w) in mesh order.
struct MorphPlan : AnimVerdict {
    struct Listed {                                           // per listed mesh (empty when its morphs go)
        std::vector<uint32_t> off;                            // num_vertices + 1 offsets into ent, relative to the mesh's first entry
        std::vector<MorphEntry> ent;                          // within a vertex ascending by target
        std::vector<double> D;                                // per target its largest |delta component|, in binary64
    };
    std::vector<Listed> listed;
    std::vector<size_t> entries;                              // per listed mesh, from the counts alone
    std::vector<uint32_t> num_targets, off_first, ent_first, w_first;      // per mesh after the call: its targets and its places
    std::vector<size_t> num_entries;                          // per mesh after the call
    size_t offs = 0, ents = 0, targets = 0;                   // of the morphed meshes
    size_t off_bytes = 0, ent_bytes = 0, w_bytes = 0;         // the device buffers (0: none)
};

// The first phase: the counts and what follows from them, before any index or delta is read
inline int plan_morph_counts(const AnimScene& sc, const char* who, const fovpt_mesh_morph* morphs, int num, MorphPlan& P)
{
    const int nmesh = (int)sc.mesh.size();
    std::vector<char> seen((size_t)nmesh, 0);
    P.entries.assign((size_t)(num > 0 ? num : 0), 0);
    for (int k = 0; k < num; k++) {
        const fovpt_mesh_morph& K = morphs[k];
        if (anim_list_mesh(P, seen, who, K.mesh)) return P.code;
        if (K._reserved) return P.refuse("%s: mesh %d: _reserved is %u", who, K.mesh, K._reserved);
        const uint32_t nv = sc.mesh[K.mesh].nv;
        if (K.num_vertices != nv) return P.refuse("%s: mesh %d has %u vertices, not %u", who, K.mesh, nv, K.num_vertices);
        if (K.num_targets > FOVPT_MORPH_MAX_TARGETS) return P.refuse("%s: mesh %d: %u targets (at most %d)", who, K.mesh, K.num_targets, FOVPT_MORPH_MAX_TARGETS);
        if (K.num_targets == 0) {
            if (K.targets) return P.refuse("%s: mesh %d: no targets, but a pointer (removing morphs takes a null pointer)", who, K.mesh);
            continue;
        }
        if (!K.targets) return P.refuse("%s: mesh %d: null targets", who, K.mesh);
        for (uint32_t t = 0; t < K.num_targets; t++) {
            const fovpt_morph_target& T = K.targets[t];
            if (T._reserved) return P.refuse("%s: mesh %d target %u: _reserved is %u", who, K.mesh, t, T._reserved);
            if (T.count > nv) return P.refuse("%s: mesh %d target %u: %u entries for %u vertices", who, K.mesh, t, T.count, nv);
            if (!T.index && T.count != 0 && T.count != nv)
                return P.refuse("%s: mesh %d target %u: no indices, but %u entries for %u vertices", who, K.mesh, t, T.count, nv);
            if (!T.delta && T.count) return P.refuse("%s: mesh %d target %u: null delta", who, K.mesh, t);
            P.entries[k] += T.count;
        }
    }
    // the new layout (its size is known from the counts alone: checked before the entries themselves are read)
    P.num_targets.assign((size_t)nmesh, 0); P.num_entries.assign((size_t)nmesh, 0);
    for (int m = 0; m < nmesh; m++) { P.num_targets[m] = sc.mesh[m].morph_targets; P.num_entries[m] = sc.mesh[m].morph_entries; }
    for (int k = 0; k < num; k++) { P.num_targets[morphs[k].mesh] = morphs[k].num_targets; P.num_entries[morphs[k].mesh] = P.entries[k]; }
    for (int m = 0; m < nmesh; m++)
        if (P.num_targets[m]) { P.offs += (size_t)sc.mesh[m].nv + 1; P.ents += P.num_entries[m]; P.targets += P.num_targets[m]; }
    if (P.ents >= (1ull << 32) || P.offs >= (1ull << 32)) return P.refuse("%s: more than 2^32 - 1 entries (%zu) or offsets (%zu)", who, P.ents, P.offs);
    return FOVPT_OK;
}

inline int plan_morphs(const AnimScene& sc, const char* who, const fovpt_mesh_morph* morphs, int num, MorphPlan& P)
{
    if (plan_morph_counts(sc, who, morphs, num, P)) return P.code;
    for (int k = 0; k < num; k++) {
        const fovpt_mesh_morph& K = morphs[k];
        for (uint32_t t = 0; t < K.num_targets; t++) {
            const fovpt_morph_target& T = K.targets[t];
            for (uint32_t i = 0; T.index && i < T.count; i++) {
                if (T.index[i] >= K.num_vertices) return P.refuse("%s: mesh %d target %u entry %u: vertex %u of %u", who, K.mesh, t, i, T.index[i], K.num_vertices);
                if (i && T.index[i] <= T.index[i - 1]) return P.refuse("%s: mesh %d target %u entry %u: indices are not strictly ascending", who, K.mesh, t, i);
            }
            for (size_t i = 0; i < 3 * (size_t)T.count; i++)
                if (!std::isfinite(T.delta[i])) return P.refuse("%s: mesh %d target %u entry %zu: a delta is not finite", who, K.mesh, t, i / 3);
        }
    }
    // the named meshes' targets, transposed: a count per vertex, its running sum, then the targets in ascending order
    P.listed.resize((size_t)(num > 0 ? num : 0));
    for (int k = 0; k < num; k++) {
        const fovpt_mesh_morph& K = morphs[k];
        MorphPlan::Listed& D = P.listed[k];
        if (!K.num_targets) continue;
        const uint32_t nv = K.num_vertices;
        D.D.assign(K.num_targets, 0.0);
        D.off.assign((size_t)nv + 1, 0);
        for (uint32_t t = 0; t < K.num_targets; t++)
            for (uint32_t i = 0; i < K.targets[t].count; i++) D.off[(K.targets[t].index ? K.targets[t].index[i] : i) + 1]++;
        for (uint32_t i = 0; i < nv; i++) D.off[i + 1] += D.off[i];
        D.ent.resize(P.entries[k]);
        std::vector<uint32_t> fill(D.off.begin(), D.off.end() - 1);
        for (uint32_t t = 0; t < K.num_targets; t++) {
            const fovpt_morph_target& T = K.targets[t];
            for (uint32_t i = 0; i < T.count; i++) {
                const float* d = T.delta + 3 * (size_t)i;
                D.ent[fill[T.index ? T.index[i] : i]++] = MorphEntry{d[0], d[1], d[2], t};
                D.D[t] = std::fmax(D.D[t], std::fmax(std::fabs((double)d[0]), std::fmax(std::fabs((double)d[1]), std::fabs((double)d[2]))));
            }
        }
    }
    const int nmesh = (int)sc.mesh.size();
    P.off_first.assign((size_t)nmesh, 0); P.ent_first.assign((size_t)nmesh, 0); P.w_first.assign((size_t)nmesh, 0);
    uint32_t off_first = 0, ent_first = 0, w_first = 0;
    for (int m = 0; m < nmesh; m++) {
        P.off_first[m] = off_first; P.ent_first[m] = ent_first; P.w_first[m] = w_first;
        if (!P.num_targets[m]) continue;
        off_first += sc.mesh[m].nv + 1; ent_first += (uint32_t)P.num_entries[m]; w_first += P.num_targets[m];
    }
    if (P.targets) { P.off_bytes = P.offs * 4; P.ent_bytes = P.ents ? P.ents * 16 : 16; P.w_bytes = P.targets * 4; }
    return FOVPT_OK;
}

// ---- fovpt_set_rig ----------------------------------------------------------------------------------------------------------
// the squared norm of a quaternion in binary64, as the rule reads it
inline bool rig_norm_ok(const float* q)
{
    const double n2 = (((double)q[0] * (double)q[0] + (double)q[1] * (double)q[1]) + (double)q[2] * (double)q[2]) + (double)q[3] * (double)q[3];
    return n2 >= 0.25 && n2 <= 4.0;
}

// Everything k_rig_pose reads is one allocation, `blob`: its sections in this order, each at a 16-byte boundary (at[]: their
// offsets).  node_chan holds per clip and node the channels of its translation, rotation and scale (-1: rest), w_chan per clip
// and RigWeights its channel (-1: zeros); the keys of all channels lie in times / values in channel order.
enum { RIG_PARENT, RIG_LEVEL, RIG_REST, RIG_NODE_CHAN, RIG_W_CHAN, RIG_CHAN, RIG_TIMES, RIG_VALUES, RIG_PAL_NODE, RIG_PAL_DST, RIG_INV_BIND,
       RIG_RIGID_NODE, RIG_WJOBS, RIG_SECTIONS };
struct RigPlan : AnimVerdict {
    std::vector<int32_t> parent;
    std::vector<uint32_t> level;                              // 0 for a root, its parent's + 1 otherwise
    std::vector<float> rest;                                  // per node 10 floats: translation, rotation, scale
    std::vector<RigBound> bound;
    std::vector<uint32_t> pal_node, pal_dst, rigid_node;      // per palette entry its node and its place in skin_pal; per rigid binding its node
    std::vector<float> inv_bind;
    std::vector<RigWeights> wjobs;
    std::vector<int32_t> node_chan, w_chan;
    std::vector<RigChannel> chan;
    std::vector<float> times, values;
    std::vector<char> blob;
    size_t at[RIG_SECTIONS] = {};
    uint32_t num_nodes = 0, num_clips = 0, num_levels = 0, threads = 64;
    size_t outs = 0;                                          // floats k_rig_pose writes: 12 per node, rigid binding and palette entry
};

// one section of the blob: appended at a 16-byte boundary, its offset returned
template <class T> size_t rig_place(std::vector<char>& blob, const std::vector<T>& v)
{
    const size_t at = (blob.size() + 15) & ~(size_t)15;
    blob.resize(at + sizeof(T) * v.size());
    if (!v.empty()) memcpy(blob.data() + at, v.data(), sizeof(T) * v.size());
    return at;
}

// Validated in the order of the description: the counts, the nodes, the bindings, then clip by clip the channels.
inline int plan_rig(const AnimScene& sc, const char* who, const fovpt_rig_desc* rig, RigPlan& P)
{
    const int nmesh = (int)sc.mesh.size();
    const uint32_t nn = rig->num_nodes;
    if (rig->_reserved0 || rig->_reserved1 || rig->_reserved2) return P.refuse("%s: a reserved field is not 0", who);
    if (nn == 0 || nn > FOVPT_RIG_MAX_NODES) return P.refuse("%s: %u nodes (1 .. %d)", who, nn, FOVPT_RIG_MAX_NODES);
    if (rig->num_clips > FOVPT_RIG_MAX_CLIPS) return P.refuse("%s: %u clips (at most %d)", who, rig->num_clips, FOVPT_RIG_MAX_CLIPS);
    if (rig->num_bindings > (uint32_t)nmesh) return P.refuse("%s: %u bindings for %d meshes", who, rig->num_bindings, nmesh);
    if (!rig->nodes || (rig->num_bindings && !rig->bindings) || (rig->num_clips && !rig->clips))
        return P.refuse("%s: a null array with a count above 0", who);
    // nodes
    P.num_nodes = nn; P.num_clips = rig->num_clips;
    P.parent.resize(nn); P.level.resize(nn); P.rest.resize(10 * (size_t)nn);
    for (uint32_t i = 0; i < nn; i++) {
        const fovpt_rig_node& N = rig->nodes[i];
        if (N.parent < -1 || N.parent >= (int32_t)i) return P.refuse("%s: node %u: parent %d (-1, or below the node's own index)", who, i, N.parent);
        float* r = P.rest.data() + 10 * (size_t)i;
        memcpy(r, N.translation, 12); memcpy(r + 3, N.rotation, 16); memcpy(r + 7, N.scale, 12);
        for (int e = 0; e < 10; e++)
            if (!std::isfinite(r[e])) return P.refuse("%s: node %u: a rest value is not finite", who, i);
        if (!rig_norm_ok(N.rotation)) return P.refuse("%s: node %u: the rest rotation's squared norm is outside [1/4, 4]", who, i);
        P.parent[i] = N.parent;
        P.level[i] = N.parent < 0 ? 0u : P.level[N.parent] + 1u;
        P.num_levels = P.level[i] + 1 > P.num_levels ? P.level[i] + 1 : P.num_levels;
    }
    // bindings
    std::vector<int> bound_at((size_t)nmesh, -1);           // per mesh its RigWeights, -2: bound without morphs, -1: not bound
    for (uint32_t k = 0; k < rig->num_bindings; k++) {
        const fovpt_rig_binding& B = rig->bindings[k];
        if (B.mesh < 0 || B.mesh >= nmesh) return P.refuse("%s: binding %u: mesh %d of %d", who, k, B.mesh, nmesh);
        if (bound_at[B.mesh] != -1) return P.refuse("%s: binding %u: mesh %d is bound twice", who, k, B.mesh);
        if (B._reserved) return P.refuse("%s: binding %u: _reserved is %u", who, k, B._reserved);
        if (B.node < -1 || B.node >= (int32_t)nn) return P.refuse("%s: binding %u: node %d of %u", who, k, B.node, nn);
        if (B.node >= 0 && B.num_joints) return P.refuse("%s: binding %u: both a node and joints", who, k);
        const uint32_t skin_joints = sc.mesh[B.mesh].skin_joints;
        const uint32_t targets = sc.mesh[B.mesh].morph_targets;
        if (B.num_joints && B.num_joints != skin_joints)
            return P.refuse("%s: binding %u: %u joints, the skin of mesh %d has %u", who, k, B.num_joints, B.mesh, skin_joints);
        if (B.node >= 0 && targets) return P.refuse("%s: binding %u: a rigid binding of mesh %d, which has morphs", who, k, B.mesh);
        if (B.node < 0 && !B.num_joints && !targets) return P.refuse("%s: binding %u: neither a node, joints nor morphs on mesh %d", who, k, B.mesh);
        if (B.num_joints && (!B.joint_nodes || !B.inverse_bind)) return P.refuse("%s: binding %u: null joint_nodes or inverse_bind", who, k);
        for (uint32_t j = 0; j < B.num_joints; j++) {
            if (B.joint_nodes[j] >= nn) return P.refuse("%s: binding %u joint %u: node %u of %u", who, k, j, (unsigned)B.joint_nodes[j], nn);
            for (int e = 0; e < 12; e++)
                if (!std::isfinite(B.inverse_bind[12 * (size_t)j + e])) return P.refuse("%s: binding %u joint %u: an inverse bind entry is not finite", who, k, j);
            P.pal_node.push_back(B.joint_nodes[j]);
            P.pal_dst.push_back(sc.mesh[B.mesh].pal_first + j);
        }
        P.inv_bind.insert(P.inv_bind.end(), B.inverse_bind, B.inverse_bind + (B.num_joints ? 12 * (size_t)B.num_joints : 0));
        RigBound D{B.mesh, 0u, B.num_joints != 0, targets != 0, B.node >= 0};
        if (D.is_rigid) { D.rigid = (uint32_t)P.rigid_node.size(); P.rigid_node.push_back((uint32_t)B.node); }
        bound_at[B.mesh] = targets ? (int)P.wjobs.size() : -2;
        if (targets) P.wjobs.push_back(RigWeights{sc.mesh[B.mesh].w_first, targets});
        P.bound.push_back(D);
    }
    // clips
    P.node_chan.assign(3 * (size_t)nn * rig->num_clips, -1); P.w_chan.assign(P.wjobs.size() * (size_t)rig->num_clips, -1);
    size_t num_times = 0, num_values = 0;
    for (uint32_t k = 0; k < rig->num_clips; k++) {
        const fovpt_rig_clip& K = rig->clips[k];
        if (K._reserved) return P.refuse("%s: clip %u: _reserved is %u", who, k, K._reserved);
        if (K.num_channels && !K.channels) return P.refuse("%s: clip %u: null channels", who, k);
        if (K.num_channels > 3 * (size_t)nn + (size_t)nmesh) return P.refuse("%s: clip %u: %u channels name a (target, path) twice", who, k, K.num_channels);
        int32_t* nc = P.node_chan.data() + 3 * (size_t)nn * k;
        int32_t* wc = P.w_chan.data() + P.wjobs.size() * (size_t)k;
        std::vector<char> weights_seen((size_t)nmesh, 0);
        for (uint32_t h = 0; h < K.num_channels; h++) {
            const fovpt_rig_channel& H = K.channels[h];
            if (H.path < FOVPT_RIG_TRANSLATION || H.path > FOVPT_RIG_WEIGHTS) return P.refuse("%s: clip %u channel %u: path %d", who, k, h, H.path);
            if (H.interpolation != FOVPT_RIG_STEP && H.interpolation != FOVPT_RIG_LINEAR)
                return P.refuse("%s: clip %u channel %u: interpolation %d", who, k, h, H.interpolation);
            size_t width;
            int32_t* slot;
            if (H.path == FOVPT_RIG_WEIGHTS) {
                if (H.target < 0 || H.target >= nmesh) return P.refuse("%s: clip %u channel %u: mesh %d of %d", who, k, h, H.target, nmesh);
                if (bound_at[H.target] < 0) return P.refuse("%s: clip %u channel %u: mesh %d is not bound or has no morphs", who, k, h, H.target);
                if (weights_seen[H.target]) return P.refuse("%s: clip %u channel %u: the weights of mesh %d twice", who, k, h, H.target);
                weights_seen[H.target] = 1;
                slot = wc + bound_at[H.target];
                width = P.wjobs[bound_at[H.target]].num_targets;
            } else {
                if (H.target < 0 || H.target >= (int32_t)nn) return P.refuse("%s: clip %u channel %u: node %d of %u", who, k, h, H.target, nn);
                slot = nc + 3 * (size_t)H.target + H.path;
                if (*slot >= 0) return P.refuse("%s: clip %u channel %u: node %d path %d twice", who, k, h, H.target, H.path);
                width = H.path == FOVPT_RIG_ROTATION ? 4 : 3;
            }
            if (H.num_keys < 1 || H.num_keys > FOVPT_RIG_MAX_KEYS) return P.refuse("%s: clip %u channel %u: %u keys (1 .. %u)", who, k, h, H.num_keys, FOVPT_RIG_MAX_KEYS);
            if (!H.times || !H.values) return P.refuse("%s: clip %u channel %u: null times or values", who, k, h);
            for (uint32_t i = 0; i < H.num_keys; i++) {
                if (!std::isfinite(H.times[i])) return P.refuse("%s: clip %u channel %u: time %u is not finite", who, k, h, i);
                if (i && !(H.times[i] > H.times[i - 1])) return P.refuse("%s: clip %u channel %u: times are not strictly ascending at key %u", who, k, h, i);
            }
            for (size_t i = 0; i < width * H.num_keys; i++)
                if (!std::isfinite(H.values[i])) return P.refuse("%s: clip %u channel %u: value %zu is not finite", who, k, h, i);
            if (H.path == FOVPT_RIG_ROTATION)
                for (uint32_t i = 0; i < H.num_keys; i++)
                    if (!rig_norm_ok(H.values + 4 * (size_t)i)) return P.refuse("%s: clip %u channel %u: key %u's squared norm is outside [1/4, 4]", who, k, h, i);
            *slot = (int32_t)P.chan.size();
            P.chan.push_back(RigChannel{(uint32_t)num_times, (uint32_t)num_values, H.num_keys, (uint32_t)H.interpolation});
            num_times += H.num_keys; num_values += width * H.num_keys;
            if (num_times >= (1ull << 32) || num_values >= (1ull << 32) || P.chan.size() >= (1ull << 31))
                return P.refuse("%s: more than 2^32 - 1 key times or values", who);
        }
    }
    // the device copy: the keys in channel order, then one allocation
    P.times.resize(num_times); P.values.resize(num_values);
    {
        size_t h = 0;
        for (uint32_t k = 0; k < rig->num_clips; k++)
            for (uint32_t i = 0; i < rig->clips[k].num_channels; i++, h++) {
                const fovpt_rig_channel& H = rig->clips[k].channels[i];
                const size_t end = h + 1 < P.chan.size() ? P.chan[h + 1].v_first : num_values;
                memcpy(P.times.data() + P.chan[h].t_first, H.times, 4 * (size_t)H.num_keys);
                memcpy(P.values.data() + P.chan[h].v_first, H.values, 4 * (end - P.chan[h].v_first));
            }
    }
    P.at[RIG_PARENT] = rig_place(P.blob, P.parent); P.at[RIG_LEVEL] = rig_place(P.blob, P.level); P.at[RIG_REST] = rig_place(P.blob, P.rest);
    P.at[RIG_NODE_CHAN] = rig_place(P.blob, P.node_chan); P.at[RIG_W_CHAN] = rig_place(P.blob, P.w_chan); P.at[RIG_CHAN] = rig_place(P.blob, P.chan);
    P.at[RIG_TIMES] = rig_place(P.blob, P.times); P.at[RIG_VALUES] = rig_place(P.blob, P.values); P.at[RIG_PAL_NODE] = rig_place(P.blob, P.pal_node);
    P.at[RIG_PAL_DST] = rig_place(P.blob, P.pal_dst); P.at[RIG_INV_BIND] = rig_place(P.blob, P.inv_bind);
    P.at[RIG_RIGID_NODE] = rig_place(P.blob, P.rigid_node); P.at[RIG_WJOBS] = rig_place(P.blob, P.wjobs);
    P.outs = 12 * ((size_t)nn + P.rigid_node.size() + P.pal_node.size());
    // one workgroup: a thread per node, palette entry and weight of the longest job
    size_t most = nn > P.pal_node.size() ? nn : P.pal_node.size();
    for (const RigWeights& w : P.wjobs) most = w.num_targets > most ? w.num_targets : most;
    P.threads = (uint32_t)(most >= FOVPT_RIG_MAX_NODES ? FOVPT_RIG_MAX_NODES : (most + 63) / 64 * 64);
    return FOVPT_OK;
}
