// rt_bvh_cost.h -- the surface-area-heuristic cost of a mesh's device tree (the definition: include/rt_mi355x.h, "mesh tree
// quality"), as the arithmetic k_bvh_cost (rt_refit.hip) and the host mirror rt_device_bvh_cost (rt_mesh_update.cpp) share: one term,
// one block's summation tree, the fold of the block sums and the last division are each written ONCE here, so the two cannot
// drift apart.  The kernel runs the block tree as an xor-butterfly instead of bvh_cost_block_sum's loop; the additions and their
// order are the same (below).  Nothing here needs HIP or any other header of the library: tests/bvh_cost_mirror.cpp compiles it alone.
//
// A node record is 128 bytes: float lo[3][4], hi[3][4] (axis-major, one float per child), uint32 c[4], 16 bytes of padding
// (DevBvhNode in rt_dev.h).  Every unit of the library is built with -ffp-contract=off: no product below is fused into a sum.
#ifndef RT_BVH_COST_H
#define RT_BVH_COST_H

#include <stdint.h>

#ifdef __HIPCC__
#define RT_COST_FN __host__ __device__ inline
#else
#define RT_COST_FN inline
#endif

#define RT_COST_BLOCK 256u              /* terms per block: one workgroup of k_bvh_cost */
#define RT_COST_LEAF 0x80000000u
#define RT_COST_DEGENERATE 1u           /* RT_MESH_QUALITY_DEGENERATE */

// half the surface area of a box in float32: d = hi - lo per axis, then (dx dy + dy dz) + dz dx
RT_COST_FN float bvh_cost_half_area(float lx, float ly, float lz, float hx, float hy, float hz)
{
    const float dx = hx - lx, dy = hy - ly, dz = hz - lz;
    return dx * dy + dy * dz + dz * dx;
}

// term(n, c) of the record at `rec` (its 32 words): 0 for an unused child (lo[0][c] is NaN, the test the tracer and the refit
// use), else the half area times the weight as ONE float32 product, converted to double
RT_COST_FN double bvh_cost_term(const float *rec, uint32_t c)
{
    const float lx = rec[c];
    if (lx != lx) return 0.0;
    uint32_t ref;
    __builtin_memcpy(&ref, rec + 24 + c, 4);
    const float w = ref & RT_COST_LEAF ? (float)(((ref >> 28) & 7u) + 1u) : 1.0f;
    return (double)(bvh_cost_half_area(lx, rec[4 + c], rec[8 + c], rec[12 + c], rec[16 + c], rec[20 + c]) * w);
}

// H_R: the half area of the root box, the min / max over the used children of the root record (NaN when it has none)
RT_COST_FN float bvh_cost_root_half_area(const float *rec)
{
    float lo[3], hi[3];
    bool any = false;
    for (uint32_t c = 0; c < 4; c++) {
        if (rec[c] != rec[c]) continue;
        for (int a = 0; a < 3; a++) {
            const float l = rec[4 * a + c], h = rec[12 + 4 * a + c];
            if (!any || l < lo[a]) lo[a] = l;
            if (!any || h > hi[a]) hi[a] = h;
        }
        any = true;
    }
    if (!any) return __builtin_nanf("");
    return bvh_cost_half_area(lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
}

// cost and flags from S and H_R: the one place the special cases are decided
RT_COST_FN void bvh_cost_finish(double S, float HR, double *cost, uint32_t *flags)
{
    const double h = (double)HR;
    const bool finite = S - S == 0.0 && h - h == 0.0;           // neither an infinity nor a NaN
    if (!finite || h == 0.0) { *cost = 0.0; *flags = RT_COST_DEGENERATE; return; }
    *cost = 1.0 + S / h;
    *flags = 0;
}

// ---- host only ---------------------------------------------------------------------------------------------------------
// One block's sum on the host: terms 256 b .. 256 b + 255 (zeros past the last), added as the balanced binary tree over the
// index bits -- stride 1 adds t1 into t0, t3 into t2, ..., stride 2 adds (t2 + t3) into (t0 + t1), ... up to stride 128 -- which
// is what the butterfly of k_bvh_cost leaves in lane 0 of wave 0 (strides 1 .. 32 inside a wave, 64 and 128 across the four waves).
inline double bvh_cost_block_sum(const void *nodes, uint64_t n_nodes, uint64_t block)
{
    double a[RT_COST_BLOCK];
    for (uint32_t i = 0; i < RT_COST_BLOCK; i++) {
        const uint64_t t = block * RT_COST_BLOCK + i;
        a[i] = t < 4 * n_nodes ? bvh_cost_term((const float *)nodes + 32 * (t >> 2), (uint32_t)(t & 3)) : 0.0;
    }
    for (uint32_t stride = 1; stride < RT_COST_BLOCK; stride *= 2)
        for (uint32_t i = 0; i < RT_COST_BLOCK; i += 2 * stride) a[i] = a[i] + a[i + stride];
    return a[0];
}
inline uint64_t bvh_cost_blocks(uint64_t n_nodes) { return (4 * n_nodes + RT_COST_BLOCK - 1) / RT_COST_BLOCK; }
// the block sums added one after the other in block order, from 0.0
inline double bvh_cost_fold(const double *partials, uint64_t n_blocks)
{
    double S = 0.0;
    for (uint64_t b = 0; b < n_blocks; b++) S = S + partials[b];
    return S;
}
// The whole definition on node records in host memory.  false: root_ref names a node record that is not there.
inline bool bvh_cost_host(const void *nodes, uint64_t n_nodes, uint32_t root_ref, double *cost, uint32_t *flags)
{
    if (root_ref & RT_COST_LEAF) { *cost = 1.0 + (double)(((root_ref >> 28) & 7u) + 1u); *flags = 0; return true; }
    if (root_ref >= n_nodes || !nodes) return false;
    double S = 0.0;
    for (uint64_t b = 0, nb = bvh_cost_blocks(n_nodes); b < nb; b++) S = S + bvh_cost_block_sum(nodes, n_nodes, b);
    bvh_cost_finish(S, bvh_cost_root_half_area((const float *)nodes + 32 * (uint64_t)root_ref), cost, flags);
    return true;
}

#endif
