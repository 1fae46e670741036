// rt_mesh_pose.h -- a posed mesh: morph targets (blend shapes) over its base positions, then linear-blend skinning of the result
// (the definitions: include/rt_mi355x.h, "morph targets" and "mesh skinning"), as the arithmetic k_mesh_pose (rt_mesh_pose.hip),
// the host mirrors rt_mesh_skin and rt_mesh_morph and the store's resolve (rt_api.cpp) share: the walk over the active targets,
// one row of one bone's transform, the blend of the four influences and the ORDER of the two -- morph, then skin
// (mesh_pose_vertex) -- are each written ONCE here, so device and host cannot drift apart.  Nothing here needs HIP or any other
// header of the library.
//
// What makes the result exact: every product and every sum is one IEEE float32 operation in the order the definition states.
// Every unit of the library is built with -ffp-contract=off; on the device the operations are __fmul_rn / __fadd_rn besides, which
// no optimisation may fuse.
#ifndef RT_MESH_POSE_H
#define RT_MESH_POSE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) && defined(__HIP_DEVICE_COMPILE__)
#define RT_POSE_FN __host__ __device__ inline
#define RT_POSE_MUL(a, b) __fmul_rn((a), (b))
#define RT_POSE_ADD(a, b) __fadd_rn((a), (b))
#else
#ifdef __HIPCC__
#define RT_POSE_FN __host__ __device__ inline
#else
#define RT_POSE_FN inline
#endif
#define RT_POSE_MUL(a, b) ((a) * (b))
#define RT_POSE_ADD(a, b) ((a) + (b))
#endif

#define RT_POSE_MAX_BONES 1024          /* RT_MESH_SKIN_MAX_BONES: 48 KB of matrices, which k_mesh_pose keeps in LDS */
#define RT_POSE_MAX_TARGETS 256         /* RT_MESH_MORPH_MAX_TARGETS: an active list is at most 2 KB */
#define RT_POSE_MORPH_BATCH 8           /* targets whose deltas are loaded before the first of them is added */

// ---- skinning ----------------------------------------------------------------------------------------------------------
// t of the definition: row r (four floats) of a bone applied to (x, y, z)
RT_POSE_FN float mesh_skin_row(const float *row, float x, float y, float z)
{
    return RT_POSE_ADD(RT_POSE_ADD(RT_POSE_ADD(RT_POSE_MUL(row[0], x), RT_POSE_MUL(row[1], y)), RT_POSE_MUL(row[2], z)), row[3]);
}

// The skinned position of one vertex: bones is the pose (12 floats a bone, wherever it lies: global memory, LDS, the host), idx and
// w the vertex's four influences, k ascending and all four always evaluated
RT_POSE_FN void mesh_skin_vertex(const float *bones, const uint16_t idx[4], const float w[4], float x, float y, float z, float p[3])
{
    for (int r = 0; r < 3; r++) {
        float acc = RT_POSE_MUL(w[0], mesh_skin_row(bones + 12 * (uint32_t)idx[0] + 4 * r, x, y, z));
        for (int k = 1; k < 4; k++) acc = RT_POSE_ADD(acc, RT_POSE_MUL(w[k], mesh_skin_row(bones + 12 * (uint32_t)idx[k] + 4 * r, x, y, z)));
        p[r] = acc;
    }
}

// ---- morph targets -----------------------------------------------------------------------------------------------------
// One entry of the ACTIVE LIST: a target whose weight is not zero.  The list is what the definition's "for t ascending over the
// targets with weights[t] != 0" walks: the skip of a zero weight is made where the list is compacted, once a pose, not per vertex.
struct MeshMorphActive { uint32_t target; float weight; };

// the active list of a frame's weights (room for n_targets entries); returns its length
inline uint32_t mesh_morph_compact(const float *weights, uint32_t n_targets, MeshMorphActive *active)
{
    uint32_t n = 0;
    for (uint32_t t = 0; t < n_targets; t++)
        if (weights[t] != 0.0f) { active[n].target = t; active[n].weight = weights[t]; n++; }      // (-0 == 0: skipped as well)
    return n;
}

// The morphed position of one vertex.  d: the vertex's delta in target 0 (deltas + 3 i); stride: floats from one target to the
// next (3 nv); active: the list, wherever it lies; p: the base position in, the morphed position out.  The loads of a batch of
// targets are independent of the sums and stand ahead of them: the adds are ordered by definition, the loads are not.
RT_POSE_FN void mesh_morph_vertex(const float *d, size_t stride, const MeshMorphActive *active, uint32_t n_active, float p[3])
{
    uint32_t k = 0;
    for (; k + RT_POSE_MORPH_BATCH <= n_active; k += RT_POSE_MORPH_BATCH) {
        float dl[RT_POSE_MORPH_BATCH][3];
#pragma unroll
        for (int j = 0; j < RT_POSE_MORPH_BATCH; j++) {
            const float *q = d + stride * active[k + j].target;
            dl[j][0] = q[0]; dl[j][1] = q[1]; dl[j][2] = q[2];
        }
#pragma unroll
        for (int j = 0; j < RT_POSE_MORPH_BATCH; j++) {
            const float w = active[k + j].weight;
            for (int c = 0; c < 3; c++) p[c] = RT_POSE_ADD(p[c], RT_POSE_MUL(w, dl[j][c]));
        }
    }
    for (; k < n_active; k++) {
        const float *q = d + stride * active[k].target;
        const float w = active[k].weight;
        for (int c = 0; c < 3; c++) p[c] = RT_POSE_ADD(p[c], RT_POSE_MUL(w, q[c]));
    }
}

// ---- a pose --------------------------------------------------------------------------------------------------------------
// THE definition of a posed vertex, i of nv: it starts from the base, the active targets are added (none: a bone pose, whose base
// is the skin's rest position, and deltas is not touched), and then, n_bones != 0, the skin is applied to what the targets left
// (none: a morph pose without bones; bones is not read).  influences(i, idx, w) fetches the vertex's own four influences the way
// its caller holds them, and is called only where there are bones, behind the targets.
template <class Influences>
RT_POSE_FN void mesh_pose_vertex(const float *base, const float *deltas, size_t nv, size_t i, const MeshMorphActive *active, uint32_t n_active,
                                 const float *bones, uint32_t n_bones, Influences influences, float p[3])
{
    const float *v = base + 3 * i;
    p[0] = v[0]; p[1] = v[1]; p[2] = v[2];
    if (n_active) mesh_morph_vertex(deltas + 3 * i, 3 * nv, active, n_active, p);
    if (n_bones) {
        uint16_t idx[4];
        float w[4], q[3];
        influences(i, idx, w);
        mesh_skin_vertex(bones, idx, w, p[0], p[1], p[2], q);
        p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
    }
}

// ---- host only ---------------------------------------------------------------------------------------------------------
// The whole definition on arrays whose entries have been checked; v_out may be v_base.  n_targets == 0: no morph set (deltas and
// weights are not read); n_bones == 0: no skin (bone_index, weight and bones are not read).
inline void mesh_pose_host(const float *v_base, uint64_t nv, const float *deltas, uint32_t n_targets, const float *weights,
                           const uint16_t *bone_index, const float *weight, const float *bones, uint32_t n_bones, float *v_out)
{
    MeshMorphActive active[RT_POSE_MAX_TARGETS];
    const uint32_t n_active = mesh_morph_compact(weights, n_targets, active);
    const auto influences = [=](size_t i, uint16_t idx[4], float w[4]) { for (int k = 0; k < 4; k++) { idx[k] = bone_index[4 * i + k]; w[k] = weight[4 * i + k]; } };
    for (uint64_t i = 0; i < nv; i++) {
        float p[3];
        mesh_pose_vertex(v_base, deltas, (size_t)nv, (size_t)i, active, n_active, bones, n_bones, influences, p);
        v_out[3 * i] = p[0]; v_out[3 * i + 1] = p[1]; v_out[3 * i + 2] = p[2];
    }
}
// the two public mirrors: skinning alone, morph targets alone
inline void mesh_skin_host(const float *v_rest, uint64_t nv, const uint16_t *bone_index, const float *weight, const float *bones, uint32_t n_bones, float *v_out)
{
    mesh_pose_host(v_rest, nv, nullptr, 0, nullptr, bone_index, weight, bones, n_bones, v_out);
}
inline void mesh_morph_host(const float *v_base, uint64_t nv, const float *deltas, uint32_t n_targets, const float *weights, float *v_out)
{
    mesh_pose_host(v_base, nv, deltas, n_targets, weights, nullptr, nullptr, nullptr, 0, v_out);
}

#endif
