// rt_mesh_pose.hip -- a mesh posed on the device that refits it, by bones, by morph targets or by both: the posed positions written
// into the buffer the refit, the device build, k_mesh_normals and k_motion_mesh read.  The definitions are in include/rt_mi355x.h
// ("mesh skinning", "morph targets"), the arithmetic and the order of the two in rt_mesh_pose.h (mesh_pose_vertex), which the
// host mirrors (rt_mesh_skin, rt_mesh_morph) and the store's resolve call as well.
//
//   k_mesh_pose      one lane per vertex, one launch a pose, whatever its kind.
//                    Morph targets: the active list -- (target, weight) of the non-zero weights, at most 2 KB -- is the same for
//                    every lane: it is read at wave-uniform addresses from a const __restrict__ kernel argument, which the
//                    compiler turns into scalar loads (the list costs no vector memory traffic and no LDS).  For each active
//                    target a lane loads its 12-byte delta (the lanes of a wave cover 768 contiguous bytes between them, so
//                    every fetched line is used whole); mesh_morph_vertex issues the loads of RT_POSE_MORPH_BATCH targets ahead
//                    of the adds that consume them, because the adds form one dependent chain and the loads do not.  A bone
//                    pose is the empty list over the skin's rest positions: no delta is touched.
//                    Bones: the workgroup first stages the pose into LDS, 16 bytes a lane and step (48 bytes a bone: three
//                    16-byte rows; 48 KB at the cap of 1024 bones), because every lane then reads four bones of its own
//                    choosing, 48 bytes each -- from LDS, not from L2.  Behind the barrier a lane loads its four indices as one
//                    8-byte and its four weights as one 16-byte access and blends over the morphed position.  Without bones
//                    nothing is staged.
//                    12 (n_active + 2) bytes a vertex read or written once (a 12-byte stride, every line used whole), + 24
//                    with a skin.
//
// No atomics, no cross-lane traffic, no divergence but the tail guard (which sits behind the barrier: every lane of the last
// workgroup stages).  One kernel, no variants: at a mesh's size it is as long as its launch.
#include <hip/hip_runtime.h>

#include "rt_launch.h"
#include "rt_mesh_pose.h"

#define RT_POSE_BLOCK 256

__global__ __launch_bounds__(RT_POSE_BLOCK) void k_mesh_pose(const float *__restrict__ base, const float *__restrict__ deltas,
                                                             const MeshMorphActive *__restrict__ active, uint32_t n_active,
                                                             const uint2 *__restrict__ bone_index, const float4 *__restrict__ weight,
                                                             const float4 *__restrict__ bones, uint32_t n_bones, uint32_t nv,
                                                             float *__restrict__ out)
{
    extern __shared__ float4 s_bones[];          // 3 n_bones rows (none without a skin)
    for (uint32_t r = threadIdx.x; r < 3u * n_bones; r += RT_POSE_BLOCK) s_bones[r] = bones[r];
    __syncthreads();
    const uint32_t i = blockIdx.x * RT_POSE_BLOCK + threadIdx.x;
    if (i >= nv) return;
    // a lane's four indices as one 8-byte and its four weights as one 16-byte access
    const auto influences = [=](size_t j, uint16_t idx[4], float w[4]) {
        const uint2 packed = bone_index[j];
        const float4 w4 = weight[j];
        idx[0] = (uint16_t)(packed.x & 0xffffu); idx[1] = (uint16_t)(packed.x >> 16); idx[2] = (uint16_t)(packed.y & 0xffffu); idx[3] = (uint16_t)(packed.y >> 16);
        w[0] = w4.x; w[1] = w4.y; w[2] = w4.z; w[3] = w4.w;
    };
    float p[3];
    mesh_pose_vertex(base, deltas, nv, i, active, n_active, (const float *)s_bones, n_bones, influences, p);
    float *o = out + 3 * (size_t)i;
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
}

hipError_t rtk_launch_mesh_pose(hipStream_t st, const MeshPoseRequest &R)
{
    if (R.nv == 0) return hipSuccess;
    if (R.n_active > RT_POSE_MAX_TARGETS || R.n_bones > RT_POSE_MAX_BONES) return hipErrorInvalidValue;
    // bones need the skin; no bones, a delta array (a pose of neither kind is no pose); an active list, both of its arrays
    if (R.n_bones ? (!R.bone_index || !R.weight || !R.bones) : !R.deltas) return hipErrorInvalidValue;
    if (R.n_active && (!R.deltas || !R.active)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mesh_pose, dim3((R.nv + RT_POSE_BLOCK - 1) / RT_POSE_BLOCK), dim3(RT_POSE_BLOCK), (size_t)R.n_bones * 48, st,
                       R.base, R.deltas, (const MeshMorphActive *)R.active, R.n_active, (const uint2 *)R.bone_index, (const float4 *)R.weight,
                       (const float4 *)R.bones, R.n_bones, R.nv, R.out);
    return hipGetLastError();
}
