// rt_bvh_build.hip -- a mesh's traversal tree built on the device that holds the mesh: a linear BVH over Morton-sorted triangles,
// collapsed four-wide into the DevBvhNode records the tracing kernels walk.  The definition is in include/rt_mi355x.h ("device
// tree build"); the arithmetic is rt_lbvh.h's, which the host mirror (rt_device_lbvh_build) is made of as well, so the two give
// the same tree.  The sort is rocPRIM's (hipcub front end); everything else is written here.
//
//   k_lbvh_cbox        one lane per face: its centroid, min / max over the wave (xor-butterfly) and over the workgroup's four waves
//                      through LDS; six floats per workgroup.  k_lbvh_cbox_fold: one workgroup folds those into the mesh's
//                      centroid box.  Min and max are order-free up to the sign of a zero, which no key depends on: no float atomics.
//   k_lbvh_keys        one lane per face: morton << 32 | face.  The keys are in face order, so a STABLE sort on the Morton bits
//                      alone (bits 32 .. 61: four 8-bit passes instead of eight) is the ascending sort of the whole keys.
//   k_lbvh_hierarchy   one lane per internal node of the binary radix tree (Karras 2012): its key range, its split, its two child refs
//                      -- a leaf from the range length alone -- and its children's parent links.  A node inside a leaf is marked dead.
//   k_lbvh_boxes       one lane per internal node that has a leaf child: the leaf boxes from the vertices, then up the parent links
//                      with one visit counter per node (two arrivals complete a node: the first arriver leaves, the second goes
//                      on).  Nothing spins, nothing waits on another workgroup.  A box crosses workgroups as plain stores behind an
//                      agent-scope fence, the counter's atomic add, and a fence again before the loads of whoever arrives last.
//                      A node's box is its left child's grown by its right child's, whoever computes it: the same bytes every run.
//   k_lbvh_collapse    ONE workgroup of 1024 lanes walks the device levels from the root: one lane per record of the level expands
//                      its binary node (lbvh_expand), a workgroup scan of the internal-child counts numbers the next level's records
//                      by (parent record, child position) -- deterministic, where an atomic append would not be -- and the lane
//                      writes its 128-byte record.  `held` goes down with the records and is max-reduced into stack_need.  The
//                      whole collapse is one launch and needs no host round trip per level: level_off comes back with the result.
//   k_lbvh_slots       one lane per slot: slot_face, the six indices of slot_idx and, with texture vertices, the 9 floats of tex.
//                      k_mesh_retri (rt_refit.hip) then writes tris and nrm as for any vertex update.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "rt_launch.h"
#include "rt_lbvh.h"

#define RT_BUILD_BLOCK 256
#define RT_COLLAPSE_BLOCK 1024

static_assert(sizeof(LbvhBin) == 56 && sizeof(DevBvhNode) == 128, "the layouts rt_lbvh.h is written for");

__device__ inline void wave_minmax6(float *b)
{
    for (int stride = 1; stride < 64; stride *= 2)
        for (int a = 0; a < 3; a++) { b[a] = lbvh_min(b[a], __shfl_xor(b[a], stride, 64)); b[3 + a] = lbvh_max(b[3 + a], __shfl_xor(b[3 + a], stride, 64)); }
}
// the workgroup's box in thread 0 (every thread calls it)
__device__ inline void block_minmax6(float *b, float (*wave_box)[6])
{
    wave_minmax6(b);
    if ((threadIdx.x & 63u) == 0) for (int k = 0; k < 6; k++) wave_box[threadIdx.x >> 6][k] = b[k];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < RT_BUILD_BLOCK / 64; w++) for (int a = 0; a < 3; a++) { b[a] = lbvh_min(b[a], wave_box[w][a]); b[3 + a] = lbvh_max(b[3 + a], wave_box[w][3 + a]); }
}

__global__ __launch_bounds__(RT_BUILD_BLOCK) void k_lbvh_cbox(const float *__restrict__ v, const uint32_t *__restrict__ f, uint32_t nf, float *__restrict__ partials)
{
    __shared__ float wave_box[RT_BUILD_BLOCK / 64][6];
    const uint32_t i = blockIdx.x * RT_BUILD_BLOCK + threadIdx.x;
    float b[6];
    lbvh_box_empty(b);
    if (i < nf) {
        float c[3];
        lbvh_centroid(v, f + 3 * (size_t)i, c);
        for (int a = 0; a < 3; a++) { b[a] = lbvh_min(b[a], c[a]); b[3 + a] = lbvh_max(b[3 + a], c[a]); }
    }
    block_minmax6(b, wave_box);
    if (threadIdx.x == 0) for (int k = 0; k < 6; k++) partials[6 * (size_t)blockIdx.x + k] = b[k];
}
// partials[0 .. n_blocks) folded into partials[n_blocks]
__global__ __launch_bounds__(RT_BUILD_BLOCK) void k_lbvh_cbox_fold(float *partials, uint32_t n_blocks)
{
    __shared__ float wave_box[RT_BUILD_BLOCK / 64][6];
    float b[6];
    lbvh_box_empty(b);
    for (uint32_t i = threadIdx.x; i < n_blocks; i += RT_BUILD_BLOCK) lbvh_box_add(b, partials + 6 * (size_t)i);
    block_minmax6(b, wave_box);
    if (threadIdx.x == 0) for (int k = 0; k < 6; k++) partials[6 * (size_t)n_blocks + k] = b[k];
}

__global__ __launch_bounds__(RT_BUILD_BLOCK) void k_lbvh_keys(const float *__restrict__ v, const uint32_t *__restrict__ f, uint32_t nf, const float *__restrict__ cbox,
                                                              unsigned long long *__restrict__ keys)
{
    const uint32_t i = blockIdx.x * RT_BUILD_BLOCK + threadIdx.x;
    if (i >= nf) return;
    float cb[6];
    for (int k = 0; k < 6; k++) cb[k] = cbox[k];
    keys[i] = lbvh_key(v, f, i, cb);
}

__global__ __launch_bounds__(RT_BUILD_BLOCK) void k_lbvh_hierarchy(const unsigned long long *__restrict__ keys, uint32_t nf, LbvhBin *__restrict__ bin, uint32_t *__restrict__ parent)
{
    const uint32_t i = blockIdx.x * RT_BUILD_BLOCK + threadIdx.x;
    if (i + 1 >= nf) return;
    uint32_t first, last, split;
    lbvh_range((const uint64_t *)keys, (int64_t)nf, (int64_t)i, &first, &last, &split);
    if (last - first + 1u <= RT_LBVH_LEAF_TRIS) { bin[i].ref[0] = RT_LBVH_DEAD; bin[i].ref[1] = RT_LBVH_DEAD; return; }
    const uint32_t l = lbvh_child_ref(first, split, split), r = lbvh_child_ref(split + 1u, last, split + 1u);
    bin[i].ref[0] = l; bin[i].ref[1] = r;
    // (a child's index lies inside this node's key range, below nf - 1: an internal child covers at least two keys)
    if (!(l & RT_LBVH_LEAF)) parent[l] = i << 1;
    if (!(r & RT_LBVH_LEAF)) parent[r] = (i << 1) | 1u;
}

__global__ __launch_bounds__(RT_BUILD_BLOCK) void k_lbvh_boxes(LbvhBin *bin, const uint32_t *__restrict__ parent, uint32_t *visit, const unsigned long long *__restrict__ keys,
                                                               const float *__restrict__ v, const uint32_t *__restrict__ f, uint32_t n_internal)
{
    const uint32_t i = blockIdx.x * RT_BUILD_BLOCK + threadIdx.x;
    if (i >= n_internal) return;
    const uint32_t r0 = bin[i].ref[0], r1 = bin[i].ref[1];
    if (r0 == RT_LBVH_DEAD) return;
    uint32_t add = 0;
    float b[6];
    if (r0 & RT_LBVH_LEAF) { lbvh_leaf_box(r0, (const uint64_t *)keys, v, f, b); for (int k = 0; k < 6; k++) bin[i].box[0][k] = b[k]; add++; }
    if (r1 & RT_LBVH_LEAF) { lbvh_leaf_box(r1, (const uint64_t *)keys, v, f, b); for (int k = 0; k < 6; k++) bin[i].box[1][k] = b[k]; add++; }
    if (add == 0) return;
    uint32_t cur = i;
    for (;;) {
        __threadfence();                                        // the boxes just stored, before the arrival that announces them
        const uint32_t old = atomicAdd(visit + cur, add);
        if (old + add < 2u) return;                             // the other child is still to come: whoever brings it goes on
        __threadfence();                                        // ... and reads what the earlier arrival stored only behind this
        float o[6];
        for (int k = 0; k < 6; k++) {
            b[k] = __uint_as_float(__hip_atomic_load((const uint32_t *)&bin[cur].box[0][k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            o[k] = __uint_as_float(__hip_atomic_load((const uint32_t *)&bin[cur].box[1][k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }
        lbvh_box_add(b, o);
        const uint32_t p = parent[cur];
        if (p == RT_LBVH_NO_PARENT) return;                     // the root's own box is nobody's child box
        cur = p >> 1;
        for (int k = 0; k < 6; k++) bin[cur].box[p & 1u][k] = b[k];
        add = 1;
    }
}

__global__ __launch_bounds__(RT_COLLAPSE_BLOCK) void k_lbvh_collapse(const LbvhBin *__restrict__ bin, uint32_t *rec_bin, int32_t *rec_held, uint4 *nodes, uint32_t cap,
                                                                     uint32_t *__restrict__ result)
{
    __shared__ uint32_t wave_tot[RT_COLLAPSE_BLOCK / 64];
    __shared__ int wave_need[RT_COLLAPSE_BLOCK / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) { rec_bin[0] = 0u; rec_held[0] = 0; result[4] = 0u; }
    __syncthreads();
    uint32_t off = 0, n = 1, level = 0, overflow = 0;
    int need = 0;
    while (n > 0 && level < RT_LBVH_MAX_LEVELS) {
        const uint32_t base = off + n;                          // where the next level's records start
        uint32_t running = 0;
        for (uint32_t s = 0; s < n; s += RT_COLLAPSE_BLOCK) {
            const bool active = s + tid < n;
            const uint32_t rec = off + s + tid;
            uint32_t ref[4]; float box[4][6];
            int nc = 0, held = 0;
            uint32_t k = 0;
            if (active) {
                nc = lbvh_expand(bin, rec_bin[rec], ref, box);
                held = rec_held[rec] + nc - 1;
                need = held > need ? held : need;
                for (int i = 0; i < nc; i++) k += (ref[i] & RT_LBVH_LEAF) ? 0u : 1u;
            }
            uint32_t incl = k;                                  // inclusive scan over the workgroup: a wave, then the wave totals
            for (int d = 1; d < 64; d *= 2) { const uint32_t t = __shfl_up(incl, d, 64); if (lane >= (uint32_t)d) incl += t; }
            if (lane == 63u) wave_tot[wave] = incl;
            __syncthreads();
            uint32_t before = 0, total = 0;
            for (uint32_t w = 0; w < RT_COLLAPSE_BLOCK / 64; w++) { const uint32_t t = wave_tot[w]; if (w < wave) before += t; total += t; }
            __syncthreads();
            if (base + running + total > cap) { overflow = 1; total = 0; }      // (uniform: never for a tree of the definition)
            else if (active) {
                uint32_t child = base + running + before + incl - k;
                for (int i = 0; i < nc; i++)
                    if (!(ref[i] & RT_LBVH_LEAF)) { rec_bin[child] = ref[i]; rec_held[child] = held; ref[i] = child++; }
                uint32_t w[32];
                lbvh_record(w, nc, ref, box);
                uint4 *out = nodes + 8 * (size_t)rec;
                for (int q = 0; q < 8; q++) out[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
            }
            running += total;
        }
        level++;
        if (tid == 0) result[4 + level] = base;
        off = base; n = running;
        __syncthreads();                                        // the next level's rec_bin / rec_held, written by other lanes of this workgroup
    }
    for (int stride = 1; stride < 64; stride *= 2) { const int t = __shfl_xor(need, stride, 64); need = t > need ? t : need; }
    if (lane == 0) wave_need[wave] = need;
    __syncthreads();
    if (tid == 0) {
        for (uint32_t w = 1; w < RT_COLLAPSE_BLOCK / 64; w++) need = wave_need[w] > need ? wave_need[w] : need;
        result[0] = off; result[1] = level; result[2] = (uint32_t)need; result[3] = (n > 0 || overflow) ? 1u : 0u;
    }
}

__global__ __launch_bounds__(RT_BUILD_BLOCK) void k_lbvh_slots(const unsigned long long *__restrict__ keys, uint32_t nf, const uint32_t *__restrict__ f, const uint32_t *__restrict__ fn,
                                                               const float *__restrict__ vt, const uint32_t *__restrict__ ft, uint32_t *__restrict__ slot_face,
                                                               uint32_t *__restrict__ slot_idx, float *__restrict__ tex)
{
    const uint32_t s = blockIdx.x * RT_BUILD_BLOCK + threadIdx.x;
    if (s >= nf) return;
    const uint32_t face = (uint32_t)keys[s];
    slot_face[s] = face;
    uint2 *I = (uint2 *)(slot_idx + 6 * (size_t)s);
    const uint32_t *a = f + 3 * (size_t)face, *b = fn + 3 * (size_t)face;
    I[0] = make_uint2(a[0], a[1]); I[1] = make_uint2(a[2], b[0]); I[2] = make_uint2(b[1], b[2]);
    if (tex) {
        float *o = tex + 9 * (size_t)s;
        for (int k = 0; k < 3; k++) {
            const float *q = vt + 3 * (size_t)ft[3 * (size_t)face + k];
            o[3 * k] = q[0]; o[3 * k + 1] = q[1]; o[3 * k + 2] = q[2];
        }
    }
}

size_t rtk_mesh_build_sort_bytes(uint32_t n_faces)
{
    size_t tmp = 0;
    hipcub::DoubleBuffer<unsigned long long> k(nullptr, nullptr);
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, tmp, k, (int)n_faces, 32, 62);
    return tmp;
}

hipError_t rtk_launch_mesh_build(hipStream_t st, const MeshBuildRequest &R, int *launches)
{
    const uint32_t nf = R.n_faces, blocks = (nf + RT_BUILD_BLOCK - 1) / RT_BUILD_BLOCK;
    const MeshBuildScratch &S = R.scratch;
    int n = 0;
    hipError_t e;
    hipLaunchKernelGGL(k_lbvh_cbox, dim3(blocks), dim3(RT_BUILD_BLOCK), 0, st, R.v, R.f, nf, S.cbox);
    hipLaunchKernelGGL(k_lbvh_cbox_fold, dim3(1), dim3(RT_BUILD_BLOCK), 0, st, S.cbox, blocks);
    hipLaunchKernelGGL(k_lbvh_keys, dim3(blocks), dim3(RT_BUILD_BLOCK), 0, st, R.v, R.f, nf, (const float *)(S.cbox + 6 * (size_t)blocks), S.keys[0]);
    hipcub::DoubleBuffer<unsigned long long> kb(S.keys[0], S.keys[1]);
    size_t tmp_bytes = S.sort_tmp_bytes;
    if ((e = hipcub::DeviceRadixSort::SortKeys(S.sort_tmp, tmp_bytes, kb, (int)nf, 32, 62, st)) != hipSuccess) return e;
    const unsigned long long *keys = kb.Current();
    n += 4;
    if (R.after_sort && (e = hipEventRecord(R.after_sort, st)) != hipSuccess) return e;
    if (nf > RT_LBVH_LEAF_TRIS) {
        const uint32_t ni = nf - 1, iblocks = (ni + RT_BUILD_BLOCK - 1) / RT_BUILD_BLOCK;
        if ((e = hipMemsetAsync(S.parent, 0xFF, (size_t)ni * 4, st)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(S.visit, 0, (size_t)ni * 4, st)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_lbvh_hierarchy, dim3(iblocks), dim3(RT_BUILD_BLOCK), 0, st, keys, nf, S.bin, S.parent);
        hipLaunchKernelGGL(k_lbvh_boxes, dim3(iblocks), dim3(RT_BUILD_BLOCK), 0, st, S.bin, (const uint32_t *)S.parent, S.visit, keys, R.v, R.f, ni);
        n += 2;
    }
    if (R.after_boxes && (e = hipEventRecord(R.after_boxes, st)) != hipSuccess) return e;
    if (nf > RT_LBVH_LEAF_TRIS) {
        hipLaunchKernelGGL(k_lbvh_collapse, dim3(1), dim3(RT_COLLAPSE_BLOCK), 0, st, (const LbvhBin *)S.bin, S.rec_bin, S.rec_held, (uint4 *)R.nodes, nf, R.result);
        n++;
    } else if ((e = hipMemsetAsync(R.result, 0, RT_LBVH_RESULT_WORDS * 4, st)) != hipSuccess) return e;
    if (R.after_collapse && (e = hipEventRecord(R.after_collapse, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_lbvh_slots, dim3(blocks), dim3(RT_BUILD_BLOCK), 0, st, keys, nf, R.f, R.fn, R.vt, R.ft, R.slot_face, R.slot_idx, R.tex);
    n++;
    if (launches) *launches = n;
    return hipGetLastError();
}
