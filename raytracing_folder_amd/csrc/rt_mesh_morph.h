// rt_mesh_morph.h -- morph targets (blend shapes) of a mesh's base positions (the definition: include/rt_mi355x.h, "morph
// targets"), as the arithmetic k_mesh_morph (rt_mesh_morph.hip) and the host mirror rt_mesh_morph (rt_api.cpp) share: the walk
// over the active targets and the chain of adds are written ONCE here, so the two cannot drift apart.  Nothing here needs HIP or
// any other header of the library.
//
// What makes the result exact: every product and every sum is one IEEE float32 operation in the order the definition states.
// Every unit of the library is built with -ffp-contract=off; on the device the operations are __fmul_rn / __fadd_rn besides, which
// no optimisation may fuse.
#ifndef RT_MESH_MORPH_H
#define RT_MESH_MORPH_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) && defined(__HIP_DEVICE_COMPILE__)
#define RT_MORPH_FN __host__ __device__ inline
#define RT_MORPH_MUL(a, b) __fmul_rn((a), (b))
#define RT_MORPH_ADD(a, b) __fadd_rn((a), (b))
#else
#ifdef __HIPCC__
#define RT_MORPH_FN __host__ __device__ inline
#else
#define RT_MORPH_FN inline
#endif
#define RT_MORPH_MUL(a, b) ((a) * (b))
#define RT_MORPH_ADD(a, b) ((a) + (b))
#endif

#define RT_MORPH_MAX_TARGETS 256        /* RT_MESH_MORPH_MAX_TARGETS: an active list is at most 2 KB */
#define RT_MORPH_BATCH 8                /* targets whose deltas are loaded before the first of them is added */

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
RT_MORPH_FN void mesh_morph_vertex(const float *d, size_t stride, const MeshMorphActive *active, uint32_t n_active, float p[3])
{
    uint32_t k = 0;
    for (; k + RT_MORPH_BATCH <= n_active; k += RT_MORPH_BATCH) {
        float dl[RT_MORPH_BATCH][3];
#pragma unroll
        for (int j = 0; j < RT_MORPH_BATCH; j++) {
            const float *q = d + stride * active[k + j].target;
            dl[j][0] = q[0]; dl[j][1] = q[1]; dl[j][2] = q[2];
        }
#pragma unroll
        for (int j = 0; j < RT_MORPH_BATCH; j++) {
            const float w = active[k + j].weight;
            for (int c = 0; c < 3; c++) p[c] = RT_MORPH_ADD(p[c], RT_MORPH_MUL(w, dl[j][c]));
        }
    }
    for (; k < n_active; k++) {
        const float *q = d + stride * active[k].target;
        const float w = active[k].weight;
        for (int c = 0; c < 3; c++) p[c] = RT_MORPH_ADD(p[c], RT_MORPH_MUL(w, q[c]));
    }
}

// ---- host only ---------------------------------------------------------------------------------------------------------
// The whole definition on arrays whose entries have been checked; v_out may be v_base
inline void mesh_morph_host(const float *v_base, uint64_t nv, const float *deltas, uint32_t n_targets, const float *weights, float *v_out)
{
    MeshMorphActive active[RT_MORPH_MAX_TARGETS];
    const uint32_t n_active = mesh_morph_compact(weights, n_targets, active);
    for (uint64_t i = 0; i < nv; i++) {
        float p[3] = {v_base[3 * i], v_base[3 * i + 1], v_base[3 * i + 2]};
        mesh_morph_vertex(deltas + 3 * i, (size_t)(3 * nv), active, n_active, p);
        v_out[3 * i] = p[0]; v_out[3 * i + 1] = p[1]; v_out[3 * i + 2] = p[2];
    }
}

#endif
