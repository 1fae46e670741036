// rt_mesh_morph.hip -- a mesh with morph targets posed on the device that refits it: the morphed (and, with bones, skinned)
// positions written into the buffer the refit, the device build, k_mesh_normals and k_motion_mesh read.  The definition is in
// include/rt_mi355x.h ("morph targets"), the arithmetic in rt_mesh_morph.h and rt_mesh_skin.h, which the host mirrors
// (rt_mesh_morph, rt_mesh_skin) call as well.
//
//   k_mesh_morph     one lane per vertex, one launch a pose.  The active list -- (target, weight) of the non-zero weights, at
//                    most 2 KB -- is the same for every lane: it is read at wave-uniform addresses from a const __restrict__
//                    kernel argument, which the compiler turns into scalar loads (the list costs no vector memory traffic and
//                    no LDS).  For each active target a lane loads its 12-byte delta (the lanes of a wave cover 768 contiguous
//                    bytes between them, so every fetched line is used whole); mesh_morph_vertex issues the loads of
//                    RT_MORPH_BATCH targets ahead of the adds that consume them, because the adds form one dependent chain
//                    and the loads do not.  With bones the workgroup first stages them into LDS exactly as k_mesh_skin does
//                    and a lane blends its four influences over the morphed position; without, nothing is staged.
//                    12 (n_active + 2) bytes a vertex read or written once, + 24 with a skin.
//
// No atomics, no cross-lane traffic, no divergence but the tail guard (which sits behind the barrier: every lane of the last
// workgroup stages).
#include <hip/hip_runtime.h>

#include "rt_launch.h"
#include "rt_mesh_morph.h"
#include "rt_mesh_skin.h"

#define RT_MORPH_BLOCK 256

__global__ __launch_bounds__(RT_MORPH_BLOCK) void k_mesh_morph(const float *__restrict__ base, const float *__restrict__ deltas,
                                                               const MeshMorphActive *__restrict__ active, uint32_t n_active,
                                                               const uint2 *__restrict__ bone_index, const float4 *__restrict__ weight,
                                                               const float4 *__restrict__ bones, uint32_t n_bones, uint32_t nv,
                                                               float *__restrict__ out)
{
    extern __shared__ float4 s_bones[];          // 3 n_bones rows (none without a skin)
    for (uint32_t r = threadIdx.x; r < 3u * n_bones; r += RT_MORPH_BLOCK) s_bones[r] = bones[r];
    __syncthreads();
    const uint32_t i = blockIdx.x * RT_MORPH_BLOCK + threadIdx.x;
    if (i >= nv) return;
    const float *v = base + 3 * (size_t)i;
    float p[3] = {v[0], v[1], v[2]};
    mesh_morph_vertex(deltas + 3 * (size_t)i, 3 * (size_t)nv, active, n_active, p);
    if (n_bones) {
        const uint2 packed = bone_index[i];
        const float4 w4 = weight[i];
        const uint16_t idx[4] = {(uint16_t)(packed.x & 0xffffu), (uint16_t)(packed.x >> 16), (uint16_t)(packed.y & 0xffffu), (uint16_t)(packed.y >> 16)};
        const float w[4] = {w4.x, w4.y, w4.z, w4.w};
        float q[3];
        mesh_skin_vertex((const float *)s_bones, idx, w, p[0], p[1], p[2], q);
        p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
    }
    float *o = out + 3 * (size_t)i;
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
}

hipError_t rtk_launch_mesh_morph(hipStream_t st, const MeshMorphRequest &R)
{
    if (R.nv == 0) return hipSuccess;
    if (R.n_active > RT_MORPH_MAX_TARGETS || R.n_bones > RT_SKIN_MAX_BONES) return hipErrorInvalidValue;
    if (R.n_bones && (!R.bone_index || !R.weight || !R.bones)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mesh_morph, dim3((R.nv + RT_MORPH_BLOCK - 1) / RT_MORPH_BLOCK), dim3(RT_MORPH_BLOCK), (size_t)R.n_bones * 48, st,
                       R.base, R.deltas, (const MeshMorphActive *)R.active, R.n_active, (const uint2 *)R.bone_index, (const float4 *)R.weight,
                       (const float4 *)R.bones, R.n_bones, R.nv, R.out);
    return hipGetLastError();
}
