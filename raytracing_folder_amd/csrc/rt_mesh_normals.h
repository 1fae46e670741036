// rt_mesh_normals.h -- the smooth vertex normals of a mesh (the definition: include/rt_mi355x.h, "smooth normals"), as the
// arithmetic k_mesh_normals (rt_mesh_normals.hip) and the host mirror rt_mesh_smooth_normals (rt_api.cpp) share: a face's
// unnormalised normal, the walk along one normal's row of corners and the last division are each written ONCE here, so the two
// cannot drift apart.  Nothing here needs HIP or any other header of the library.
//
// What makes the result exact: a float sum depends on the order of its additions and on nothing else.  ComputeNormals adds the
// faces to a vertex in face order; a row of the adjacency lists the corners of one normal in ascending order, which is face
// order; so ONE lane that walks ONE row performs the additions ComputeNormals performs for that normal, in its order -- no two
// lanes ever add into the same sum, and there is nothing for an atomic to order.  Every unit of the library is built with
// -ffp-contract=off: no product below is fused into a sum.
#ifndef RT_MESH_NORMALS_H
#define RT_MESH_NORMALS_H

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define RT_NORMALS_FN __host__ __device__ inline
#else
#define RT_NORMALS_FN inline
#endif

// N_i of face i: cross(v[f1] - v[f0], v[f2] - v[f0]) as k_mesh_retri and rt::Point3 compute it
RT_NORMALS_FN void mesh_face_normal(const float *v, const uint32_t *f, uint32_t i, float N[3])
{
    const uint32_t *fi = f + 3 * (uint64_t)i;
    const float *a = v + 3 * (uint64_t)fi[0], *b = v + 3 * (uint64_t)fi[1], *c = v + 3 * (uint64_t)fi[2];
    const float ax = a[0], ay = a[1], az = a[2];
    const float ux = b[0] - ax, uy = b[1] - ay, uz = b[2] - az;
    const float wx = c[0] - ax, wy = c[1] - ay, wz = c[2] - az;
    N[0] = uy * wz - uz * wy; N[1] = uz * wx - ux * wz; N[2] = ux * wy - uy * wx;
}

// S / |S|: false (nothing written) when the length is 0 or not finite -- the normal keeps its stored value
RT_NORMALS_FN bool mesh_normal_finish(const float S[3], float out[3])
{
    const float len = sqrtf(S[0] * S[0] + S[1] * S[1] + S[2] * S[2]);
    if (!(len > 0.0f) || len - len != 0.0f) return false;
    out[0] = S[0] / len; out[1] = S[1] / len; out[2] = S[2] / len;
    return true;
}

// Normal j from its row corners[begin .. end) (ascending): false for an empty row or a sum without a direction
RT_NORMALS_FN bool mesh_smooth_normal(const float *v, const uint32_t *f, const uint32_t *corners, uint32_t begin, uint32_t end, float out[3])
{
    if (begin == end) return false;
    float S[3] = {0.0f, 0.0f, 0.0f};
    for (uint32_t r = begin; r < end; r++) {
        float N[3];
        mesh_face_normal(v, f, corners[r] / 3u, N);
        S[0] = S[0] + N[0]; S[1] = S[1] + N[1]; S[2] = S[2] + N[2];
    }
    return mesh_normal_finish(S, out);
}

// ---- host only ---------------------------------------------------------------------------------------------------------
// The adjacency over normal indices in CSR form, by a counting sort that follows the faces: off[nvn + 1], and corner[3 nf] with
// the corners of a row ascending (they are placed in ascending order).  fn's entries are below nvn (the caller checked).
inline void mesh_normal_adjacency(const uint32_t *fn, uint64_t nf, uint64_t nvn, uint32_t *off, uint32_t *corner)
{
    for (uint64_t j = 0; j <= nvn; j++) off[j] = 0;
    for (uint64_t c = 0; c < 3 * nf; c++) off[fn[c] + 1]++;
    for (uint64_t j = 0; j < nvn; j++) off[j + 1] += off[j];
    for (uint64_t c = 0; c < 3 * nf; c++) corner[off[fn[c]]++] = (uint32_t)c;      // off[j] now ends row j: shift back
    for (uint64_t j = nvn; j > 0; j--) off[j] = off[j - 1];
    off[0] = 0;
}

#endif
