// rt_refit.hip -- mesh vertex updates in place: new vertices for a mesh whose faces stay, without building its tree again.  The
// definition is in include/rt_mi355x.h ("mesh vertex updates"); the reference has no counterpart (it loads a mesh once).  What
// makes it exact: any bounding hierarchy over the same triangles gives the same closest hit, and every box of the device tree is a
// float min / max of vertex coordinates with no rounding anywhere (rt_lower.cpp, build_sah_bvh) -- so a tree whose boxes are set
// again to the min / max of what lies beneath them is, box for box, what a fresh build would put on the same topology.
//
//   k_mesh_retri        one lane per triangle slot: its face's six indices (24 bytes, three 8-byte loads), the three vertices and
//                       three normals gathered through them, N = cross(B - A, C - A) / |..| operation by operation as
//                       upload_scene computes it on the host (this unit is built with -ffp-contract=off like the others; / and
//                       sqrtf are correctly rounded), then the slot's 48-byte DevTri as three 16-byte stores and its 36 bytes of nrm.
//   k_bvh_refit_level   one lane per (node, child) of ONE level of the tree, the levels launched deepest first on one stream: a
//                       leaf child's box is the min / max over the vertices of its (at most four) slots, read from the DevTri
//                       records k_mesh_retri has just written (three 16-byte loads a slot); an internal child's box is the
//                       fminf / fmaxf union of that node's four child boxes, which the launch before this one finished (its
//                       128-byte record's 96 bytes of boxes: six 16-byte loads; NaN boxes of unused children fall out of fminf /
//                       fmaxf).  A child whose box is NaN is unused and stays so: the boxes of used children are never NaN (the
//                       min / max start from +-3.0e38 like the host's and a NaN coordinate falls out).  Refs are never written.
//                       A bound equal to the stored one is left alone, so the sign of a zero bound stays the build's: the host's fold
//                       keeps the first of -0 and +0 it meets, in an order the refit cannot know; fminf / fmaxf would pick by sign.
//
//   k_bvh_cost          the surface-area-heuristic cost of the tree as it sits on the device (rt_mi355x.h, "mesh tree quality"): one
//                       lane per (node, child) over ALL levels at once, 256 lanes a workgroup like k_bvh_refit_level.  A lane reads
//                       its child's six bounds and its ref (seven 4-byte loads, 128 bytes a node between the four lanes of a
//                       node) and forms its term in float32 (bvh_cost_term, rt_bvh_cost.h -- the host mirror calls the same
//                       function), converts it to double, and the workgroup adds its 256 doubles in the FIXED order the header
//                       writes down: an xor-butterfly over the lane index inside each wave (strides 1 .. 32; a double travels as
//                       two 32-bit ds_bpermute), which leaves in lane 0 the balanced tree ((t0 + t1) + (t2 + t3)) + ..., then the
//                       four wave sums through 32 bytes of LDS as (w0 + w1) + (w2 + w3) -- strides 64 and 128 of the same tree.
//                       One double per workgroup goes to the partials buffer; the host adds those in index order after one small
//                       copy (RT_COST_FOLD_DEVICE: k_bvh_cost_fold does it in one lane instead -- the alternative that was
//                       measured and not kept).  No atomics, nothing that waits: IEEE additions in an order that
//                       does not depend on scheduling, so the same records give the same eight bytes on every launch and on the host.
//
// The refit is one launch per level, nothing else: no cross-workgroup synchronisation, no atomics, nothing that waits.  Min and max do not depend
// on the order of their operands, so identical inputs give identical bytes.  The four lanes of a node write disjoint floats of its
// record (lo[a][child], hi[a][child]) and read only records of the level below.
#include <hip/hip_runtime.h>

#include "rt_launch.h"
#include "rt_bvh_cost.h"

#define RT_REFIT_BLOCK 256
#define RT_REFIT_LEAF 0x80000000u

__global__ __launch_bounds__(RT_REFIT_BLOCK) void k_mesh_retri(const float *__restrict__ v, const float *__restrict__ vn, const uint32_t *__restrict__ slot_idx,
                                                               uint32_t n_slots, DevTri *__restrict__ tris, float *__restrict__ nrm)
{
    const uint32_t s = blockIdx.x * RT_REFIT_BLOCK + threadIdx.x;
    if (s >= n_slots) return;
    const uint2 *I = (const uint2 *)(slot_idx + 6 * (size_t)s);
    const uint2 i0 = I[0], i1 = I[1], i2 = I[2];              // v: i0.x, i0.y, i1.x    vn: i1.y, i2.x, i2.y
    const float *a = v + 3 * (size_t)i0.x, *b = v + 3 * (size_t)i0.y, *c = v + 3 * (size_t)i1.x;
    const float ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2], cx = c[0], cy = c[1], cz = c[2];
    // rt::Point3: (P1 - P0).Cross(P2 - P0), then Normalize() = each component / sqrtf(x x + y y + z z), sums left to right
    const float ux = bx - ax, uy = by - ay, uz = bz - az;
    const float wx = cx - ax, wy = cy - ay, wz = cz - az;
    const float nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    const float len = sqrtf(nx * nx + ny * ny + nz * nz);
    // (a triangle without area has N = 0 / 0 here as on the host: a NaN either way, whose sign bit the two need not agree on)
    float4 *T = (float4 *)(tris + s);
    T[0] = make_float4(ax, ay, az, bx);
    T[1] = make_float4(by, bz, cx, cy);
    T[2] = make_float4(cz, nx / len, ny / len, nz / len);
    const uint32_t ni[3] = {i1.y, i2.x, i2.y};
    float *o = nrm + 9 * (size_t)s;
    for (int k = 0; k < 3; k++) {
        const float *q = vn + 3 * (size_t)ni[k];
        o[3 * k] = q[0]; o[3 * k + 1] = q[1]; o[3 * k + 2] = q[2];
    }
}

__global__ __launch_bounds__(RT_REFIT_BLOCK) void k_bvh_refit_level(DevBvhNode *nodes, const uint32_t *__restrict__ level, uint32_t n_level,
                                                                    const DevTri *__restrict__ tris)
{
    const uint32_t t = blockIdx.x * RT_REFIT_BLOCK + threadIdx.x;
    if (t >= 4 * n_level) return;
    DevBvhNode *n = nodes + level[t >> 2];
    const uint32_t ch = t & 3;
    const float was = n->lo[0][ch];
    if (was != was) return;                                     // an unused child: NaN bounds, never entered
    const uint32_t ref = n->c[ch];
    float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    if (ref & RT_REFIT_LEAF) {
        const uint32_t first = ref & 0x0FFFFFFFu, cnt = ((ref >> 28) & 7u) + 1;
        for (uint32_t k = 0; k < cnt; k++) {
            const float4 *T = (const float4 *)(tris + first + k);
            const float4 p = T[0], q = T[1], r = T[2];          // A.xyz B.x | B.yz C.xy | C.z N.xyz
            lo[0] = fminf(fminf(fminf(lo[0], p.x), p.w), q.z); hi[0] = fmaxf(fmaxf(fmaxf(hi[0], p.x), p.w), q.z);
            lo[1] = fminf(fminf(fminf(lo[1], p.y), q.x), q.w); hi[1] = fmaxf(fmaxf(fmaxf(hi[1], p.y), q.x), q.w);
            lo[2] = fminf(fminf(fminf(lo[2], p.z), q.y), r.x); hi[2] = fmaxf(fmaxf(fmaxf(hi[2], p.z), q.y), r.x);
        }
    } else {
        const float4 *B = (const float4 *)(nodes + ref);        // lo[3][4], hi[3][4]: one float4 per axis and side
        for (int a = 0; a < 3; a++) {
            const float4 l = B[a], h = B[3 + a];
            lo[a] = fminf(fminf(fminf(fminf(lo[a], l.x), l.y), l.z), l.w);
            hi[a] = fmaxf(fmaxf(fmaxf(fmaxf(hi[a], h.x), h.y), h.z), h.w);
        }
    }
    // a bound that compares equal to the one already there leaves it as it is: only the sign of a zero can differ then (fminf
    // takes -0 of +-0; the host's fold keeps whichever came first), so an update that does not move a bound does not touch it
    for (int a = 0; a < 3; a++) {
        const float ol = n->lo[a][ch], oh = n->hi[a][ch];
        n->lo[a][ch] = lo[a] == ol ? ol : lo[a];
        n->hi[a][ch] = hi[a] == oh ? oh : hi[a];
    }
}

hipError_t rtk_launch_mesh_refit(hipStream_t st, const MeshRefitRequest &R)
{
    if (R.n_slots == 0) return hipSuccess;
    hipLaunchKernelGGL(k_mesh_retri, dim3((R.n_slots + RT_REFIT_BLOCK - 1) / RT_REFIT_BLOCK), dim3(RT_REFIT_BLOCK), 0, st,
                       R.v, R.vn, R.slot_idx, R.n_slots, R.tris, R.nrm);
    if (R.after_retri) { const hipError_t e = hipEventRecord(R.after_retri, st); if (e != hipSuccess) return e; }
    for (int k = 0; k < R.n_levels; k++) {
        const uint32_t n = R.level_off[k + 1] - R.level_off[k];
        if (n == 0) continue;
        hipLaunchKernelGGL(k_bvh_refit_level, dim3((4 * n + RT_REFIT_BLOCK - 1) / RT_REFIT_BLOCK), dim3(RT_REFIT_BLOCK), 0, st,
                           R.nodes, R.level_nodes + R.level_off[k], n, (const DevTri *)R.tris);
    }
    return hipGetLastError();
}

static_assert(RT_REFIT_BLOCK == RT_COST_BLOCK && RT_REFIT_BLOCK == 4 * 64, "a block of the cost's summation order is one workgroup of four waves");

__global__ __launch_bounds__(RT_REFIT_BLOCK) void k_bvh_cost(const DevBvhNode *__restrict__ nodes, uint32_t n_terms, double *__restrict__ partials)
{
    __shared__ double wave_sum[RT_REFIT_BLOCK / 64];
    const uint32_t t = blockIdx.x * RT_REFIT_BLOCK + threadIdx.x;
    // every lane stays to the end: the lanes past the last term carry the zeros the definition pads a short block with
    double x = t < n_terms ? bvh_cost_term((const float *)(nodes + (t >> 2)), t & 3u) : 0.0;
    for (int stride = 1; stride < 64; stride *= 2) x = x + __shfl_xor(x, stride, 64);
    if ((threadIdx.x & 63u) == 0) wave_sum[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

#if RT_COST_FOLD_DEVICE
// the block sums added in index order by one lane, into the slot behind them
__global__ void k_bvh_cost_fold(double *partials, uint32_t n_blocks)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double S = 0.0;
    for (uint32_t b = 0; b < n_blocks; b++) S = S + partials[b];
    partials[n_blocks] = S;
}
#endif

hipError_t rtk_launch_bvh_cost(hipStream_t st, const BvhCostRequest &R)
{
    if (R.n_nodes == 0) return hipSuccess;
    const uint32_t n_terms = 4 * R.n_nodes, n_blocks = (n_terms + RT_REFIT_BLOCK - 1) / RT_REFIT_BLOCK;
    hipLaunchKernelGGL(k_bvh_cost, dim3(n_blocks), dim3(RT_REFIT_BLOCK), 0, st, R.nodes, n_terms, R.partials);
#if RT_COST_FOLD_DEVICE
    hipLaunchKernelGGL(k_bvh_cost_fold, dim3(1), dim3(64), 0, st, R.partials, n_blocks);
#endif
    return hipGetLastError();
}
