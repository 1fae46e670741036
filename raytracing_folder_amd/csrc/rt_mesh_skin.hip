// rt_mesh_skin.hip -- a skinned mesh posed on the device that refits it: the posed positions written into the buffer the refit, the
// device build, k_mesh_normals and k_motion_mesh read.  The definition is in include/rt_mi355x.h ("mesh skinning"), the
// arithmetic in rt_mesh_skin.h, which the host mirror (rt_mesh_skin) calls as well.
//
//   k_mesh_skin      one lane per vertex.  The workgroup first stages the pose into LDS, 16 bytes a lane and step (48 bytes a bone:
//                    three 16-byte rows; 48 KB at the cap of 1024 bones), because every lane then reads four bones of its own
//                    choosing, 48 bytes each -- from LDS, not from L2.  Behind the barrier a lane loads its four indices as one
//                    8-byte and its four weights as one 16-byte access, its rest position as three 4-byte ones (a 12-byte
//                    stride: the lanes of a wave cover 768 contiguous bytes between them, so every fetched line is used whole),
//                    blends, and writes three floats the same way.  48 bytes a vertex, read or written once.
//
// No atomics, no cross-lane traffic, no divergence but the tail guard (which sits behind the barrier: every lane of the last
// workgroup stages).  One kernel, no variants: at a mesh's size it is as long as its launch.
#include <hip/hip_runtime.h>

#include "rt_launch.h"
#include "rt_mesh_skin.h"

#define RT_SKIN_BLOCK 256

__global__ __launch_bounds__(RT_SKIN_BLOCK) void k_mesh_skin(const float *__restrict__ rest, const uint2 *__restrict__ bone_index,
                                                             const float4 *__restrict__ weight, const float4 *__restrict__ bones,
                                                             uint32_t n_bones, uint32_t nv, float *__restrict__ out)
{
    extern __shared__ float4 s_bones[];          // 3 n_bones rows
    for (uint32_t r = threadIdx.x; r < 3u * n_bones; r += RT_SKIN_BLOCK) s_bones[r] = bones[r];
    __syncthreads();
    const uint32_t i = blockIdx.x * RT_SKIN_BLOCK + threadIdx.x;
    if (i >= nv) return;
    const uint2 packed = bone_index[i];
    const float4 w4 = weight[i];
    const uint16_t idx[4] = {(uint16_t)(packed.x & 0xffffu), (uint16_t)(packed.x >> 16), (uint16_t)(packed.y & 0xffffu), (uint16_t)(packed.y >> 16)};
    const float w[4] = {w4.x, w4.y, w4.z, w4.w};
    const float *v = rest + 3 * (size_t)i;
    float p[3];
    mesh_skin_vertex((const float *)s_bones, idx, w, v[0], v[1], v[2], p);
    float *o = out + 3 * (size_t)i;
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
}

hipError_t rtk_launch_mesh_skin(hipStream_t st, const MeshSkinRequest &R)
{
    if (R.nv == 0) return hipSuccess;
    if (R.n_bones == 0 || R.n_bones > RT_SKIN_MAX_BONES) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mesh_skin, dim3((R.nv + RT_SKIN_BLOCK - 1) / RT_SKIN_BLOCK), dim3(RT_SKIN_BLOCK), (size_t)R.n_bones * 48, st,
                       R.rest, (const uint2 *)R.bone_index, (const float4 *)R.weight, (const float4 *)R.bones, R.n_bones, R.nv, R.out);
    return hipGetLastError();
}
