// rt_mesh_skin.h -- linear-blend skinning of a mesh's rest pose (the definition: include/rt_mi355x.h, "mesh skinning"), as the
// arithmetic k_mesh_skin (rt_mesh_skin.hip) and the host mirror rt_mesh_skin (rt_api.cpp) share: one row of one bone's transform
// and the blend of the four influences are each written ONCE here, so the two cannot drift apart.  Nothing here needs HIP or any
// other header of the library.
//
// What makes the result exact: every product and every sum is one IEEE float32 operation in the order the definition states.
// Every unit of the library is built with -ffp-contract=off; on the device the operations are __fmul_rn / __fadd_rn besides, which
// no optimisation may fuse.
#ifndef RT_MESH_SKIN_H
#define RT_MESH_SKIN_H

#include <stdint.h>

#if defined(__HIPCC__) && defined(__HIP_DEVICE_COMPILE__)
#define RT_SKIN_FN __host__ __device__ inline
#define RT_SKIN_MUL(a, b) __fmul_rn((a), (b))
#define RT_SKIN_ADD(a, b) __fadd_rn((a), (b))
#else
#ifdef __HIPCC__
#define RT_SKIN_FN __host__ __device__ inline
#else
#define RT_SKIN_FN inline
#endif
#define RT_SKIN_MUL(a, b) ((a) * (b))
#define RT_SKIN_ADD(a, b) ((a) + (b))
#endif

#define RT_SKIN_MAX_BONES 1024          /* RT_MESH_SKIN_MAX_BONES: 48 KB of matrices, which k_mesh_skin keeps in LDS */

// t of the definition: row r (four floats) of a bone applied to (x, y, z)
RT_SKIN_FN float mesh_skin_row(const float *row, float x, float y, float z)
{
    return RT_SKIN_ADD(RT_SKIN_ADD(RT_SKIN_ADD(RT_SKIN_MUL(row[0], x), RT_SKIN_MUL(row[1], y)), RT_SKIN_MUL(row[2], z)), row[3]);
}

// The posed position of one vertex: bones is the pose (12 floats a bone, wherever it lies: global memory, LDS, the host), idx and
// w the vertex's four influences, k ascending and all four always evaluated
RT_SKIN_FN void mesh_skin_vertex(const float *bones, const uint16_t idx[4], const float w[4], float x, float y, float z, float p[3])
{
    for (int r = 0; r < 3; r++) {
        float acc = RT_SKIN_MUL(w[0], mesh_skin_row(bones + 12 * (uint32_t)idx[0] + 4 * r, x, y, z));
        for (int k = 1; k < 4; k++) acc = RT_SKIN_ADD(acc, RT_SKIN_MUL(w[k], mesh_skin_row(bones + 12 * (uint32_t)idx[k] + 4 * r, x, y, z)));
        p[r] = acc;
    }
}

// ---- host only ---------------------------------------------------------------------------------------------------------
// The whole definition on arrays whose entries have been checked; v_out may be v_rest
inline void mesh_skin_host(const float *v_rest, uint64_t nv, const uint16_t *bone_index, const float *weight, const float *bones, float *v_out)
{
    for (uint64_t i = 0; i < nv; i++) {
        float p[3];
        mesh_skin_vertex(bones, bone_index + 4 * i, weight + 4 * i, v_rest[3 * i], v_rest[3 * i + 1], v_rest[3 * i + 2], p);
        v_out[3 * i] = p[0]; v_out[3 * i + 1] = p[1]; v_out[3 * i + 2] = p[2];
    }
}

#endif
