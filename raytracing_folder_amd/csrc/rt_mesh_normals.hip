// rt_mesh_normals.hip -- the smooth vertex normals of a deforming mesh, computed again from its new positions on the device that
// refits it.  The definition is in include/rt_mi355x.h ("smooth normals"), the arithmetic in rt_mesh_normals.h, which the host
// mirror (rt_mesh_smooth_normals) calls as well.
//
//   k_mesh_normals      one lane per normal j: it walks its row of the adjacency (the corners that name j, ascending; two 4-byte
//                       loads for the row's bounds, one per corner), and for every corner forms the face's unnormalised normal
//                       from the face's three indices and three vertices (mesh_face_normal: 12 + 36 bytes a corner, from arrays a
//                       mesh of this kind keeps in L2) and adds it to its own sum, in row order.  Then S / |S| as three 4-byte
//                       stores into vn[3 j ..] -- or no store at all for a normal that is to keep its stored value (no corner, or
//                       a sum without a direction).  The lanes of a wave walk rows of different lengths: a wave takes as long as
//                       its longest row (valence about 6 on a regular mesh; a pole of valence 70 holds its wave for 70 steps).
//
// No atomics, nothing that waits, no LDS: a normal's sum lives in the registers of ONE lane and its additions are IEEE additions
// in the order the adjacency fixes, so the same mesh gives the same bytes on every launch and on the host.  Staging N_i per face
// in a launch of its own and reading it back per corner is the alternative; DESIGN.md section 3 says why it is not built.
#include <hip/hip_runtime.h>

#include "rt_launch.h"
#include "rt_mesh_normals.h"

#define RT_NORMALS_BLOCK 256

__global__ __launch_bounds__(RT_NORMALS_BLOCK) void k_mesh_normals(const float *__restrict__ v, const uint32_t *__restrict__ f,
                                                                   const uint32_t *__restrict__ nadj_off, const uint32_t *__restrict__ nadj_corner,
                                                                   uint32_t n_normals, float *__restrict__ vn)
{
    const uint32_t j = blockIdx.x * RT_NORMALS_BLOCK + threadIdx.x;
    if (j >= n_normals) return;
    float n[3];
    if (!mesh_smooth_normal(v, f, nadj_corner, nadj_off[j], nadj_off[j + 1], n)) return;
    float *o = vn + 3 * (size_t)j;
    o[0] = n[0]; o[1] = n[1]; o[2] = n[2];
}

hipError_t rtk_launch_mesh_normals(hipStream_t st, const MeshNormalsRequest &R)
{
    if (R.n_normals == 0) return hipSuccess;
    hipLaunchKernelGGL(k_mesh_normals, dim3((R.n_normals + RT_NORMALS_BLOCK - 1) / RT_NORMALS_BLOCK), dim3(RT_NORMALS_BLOCK), 0, st,
                       R.v, R.f, R.nadj_off, R.nadj_corner, R.n_normals, R.vn);
    return hipGetLastError();
}
