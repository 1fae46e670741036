// rt_lbvh.h -- the tree a device builds for a mesh by itself (the definition: include/rt_mi355x.h, "device tree build"), as the
// arithmetic the kernels of rt_bvh_build.hip and the host mirror rt_device_lbvh_build (rt_mesh_update.cpp) share: a triangle's box and
// centroid, its key, the binary radix tree over the sorted keys (Karras 2012), the four-wide collapse of one node and its
// 128-byte record are each written ONCE here, so the two cannot drift apart.  Nothing here needs HIP or any other header of the
// library: tests/lbvh_mirror_driver.cpp compiles it alone.  Every unit is built with -ffp-contract=off: no product is fused into a sum.
//
// Every minimum and maximum below is `b < a ? b : a` / `b > a ? b : a` with a the value held so far -- std::min / std::max as
// build_sah_bvh uses them: a NaN operand falls out, and of two zeros the one held stays.  A box is six floats, lo[3] then hi[3].
//
// Within a leaf the triangle slots are in KEY order, not in face order as in the host builder's leaves: the closest hit is the
// same (any bounding hierarchy over the same triangles gives it); only two triangles at a bit-equal closest t could show the difference.
#ifndef RT_LBVH_H
#define RT_LBVH_H

#include <stdint.h>

#ifdef __HIPCC__
#define RT_LBVH_FN __host__ __device__ inline
#else
#define RT_LBVH_FN inline
#endif

#define RT_LBVH_LEAF 0x80000000u
#define RT_LBVH_DEAD 0xFFFFFFFFu        /* LbvhBin::ref[0] of a binary node that lies inside a leaf (no leaf ref has a count of 8) */
#define RT_LBVH_LEAF_TRIS 4u
#define RT_LBVH_NO_PARENT 0xFFFFFFFFu

// One internal node of the binary radix tree that is not inside a leaf: its two children -- a leaf ref (bit 31, count - 1 in bits
// 28-30, first slot in bits 0-27) or the index of another internal node -- and their boxes.
struct LbvhBin { uint32_t ref[2]; float box[2][6]; };

RT_LBVH_FN float lbvh_min(float a, float b) { return b < a ? b : a; }
RT_LBVH_FN float lbvh_max(float a, float b) { return b > a ? b : a; }
RT_LBVH_FN uint32_t lbvh_leafref(uint32_t off, uint32_t cnt) { return RT_LBVH_LEAF | ((cnt - 1u) << 28) | (off & 0x0FFFFFFFu); }

RT_LBVH_FN void lbvh_box_empty(float *box) { for (int a = 0; a < 3; a++) { box[a] = 3.0e38f; box[3 + a] = -3.0e38f; } }
// box grows by the three vertices of the face whose indices are at f3
RT_LBVH_FN void lbvh_box_add_face(float *box, const float *v, const uint32_t *f3)
{
    for (int k = 0; k < 3; k++) {
        const float *q = v + 3 * (uint64_t)f3[k];
        for (int a = 0; a < 3; a++) { box[a] = lbvh_min(box[a], q[a]); box[3 + a] = lbvh_max(box[3 + a], q[a]); }
    }
}
// box grows by another box: `box` is the value held so far
RT_LBVH_FN void lbvh_box_add(float *box, const float *other)
{
    for (int a = 0; a < 3; a++) { box[a] = lbvh_min(box[a], other[a]); box[3 + a] = lbvh_max(box[3 + a], other[3 + a]); }
}
// the centroid of a face: 0.5f * (lo + hi) of its box (build_sah_bvh's TB::c)
RT_LBVH_FN void lbvh_centroid(const float *v, const uint32_t *f3, float c[3])
{
    float box[6];
    lbvh_box_empty(box);
    lbvh_box_add_face(box, v, f3);
    for (int a = 0; a < 3; a++) c[a] = 0.5f * (box[a] + box[3 + a]);
}

// one axis of a key: clamp((int)((c - clo) * (1024.0f / (chi - clo))), 0, 1023); 0 when chi - clo is not > 0 or not finite.
// (A product that is NaN or not positive gives 0 and one of 1023 or more gives 1023 without a conversion that C leaves undefined.)
RT_LBVH_FN uint32_t lbvh_quant(float c, float clo, float chi)
{
    const float ext = chi - clo;
    if (!(ext > 0.0f) || ext - ext != 0.0f) return 0u;
    const float x = (c - clo) * (1024.0f / ext);
    if (!(x > 0.0f)) return 0u;
    if (x >= 1023.0f) return 1023u;
    return (uint32_t)(int)x;
}
RT_LBVH_FN uint32_t lbvh_spread10(uint32_t x)               // bit i of 10 bits to bit 3 i
{
    x &= 0x3FFu;
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}
// the 30-bit Morton code: x in the highest bit of every triple, then y, then z
RT_LBVH_FN uint32_t lbvh_morton(uint32_t qx, uint32_t qy, uint32_t qz) { return (lbvh_spread10(qx) << 2) | (lbvh_spread10(qy) << 1) | lbvh_spread10(qz); }
// the key of a face: its Morton code above its own index, so no two keys are equal.  cbox: the box of all centroids.
RT_LBVH_FN uint64_t lbvh_key(const float *v, const uint32_t *f, uint32_t face, const float *cbox)
{
    float c[3];
    lbvh_centroid(v, f + 3 * (uint64_t)face, c);
    const uint32_t m = lbvh_morton(lbvh_quant(c[0], cbox[0], cbox[3]), lbvh_quant(c[1], cbox[1], cbox[4]), lbvh_quant(c[2], cbox[2], cbox[5]));
    return ((uint64_t)m << 32) | face;
}

// delta(i, j): the length of the common prefix of keys i and j, -1 when j is out of range
RT_LBVH_FN int lbvh_delta(const uint64_t *keys, int64_t n, int64_t i, int64_t j)
{
    if (j < 0 || j >= n) return -1;
    return __builtin_clzll(keys[i] ^ keys[j]);              // (the keys differ: the argument is never 0)
}
// Internal node i of the binary radix tree over n >= 2 sorted keys (0 <= i < n - 1; the root is 0): the key range [first, last] it
// covers and its split -- the left child covers [first, split], the right [split + 1, last]; a child that covers more than one
// key is internal node `split` (left) or `split + 1` (right).
RT_LBVH_FN void lbvh_range(const uint64_t *keys, int64_t n, int64_t i, uint32_t *first, uint32_t *last, uint32_t *split)
{
    const int d = lbvh_delta(keys, n, i, i + 1) - lbvh_delta(keys, n, i, i - 1) < 0 ? -1 : 1;
    const int dmin = lbvh_delta(keys, n, i, i - d);
    int64_t lmax = 2;
    while (lbvh_delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (lbvh_delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = lbvh_delta(keys, n, i, j);
    int64_t s = 0;
    for (int64_t t = (l + 1) / 2; ; t = (t + 1) / 2) {
        if (lbvh_delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
        if (t <= 1) break;
    }
    const int64_t g = i + s * d + (d < 0 ? -1 : 0);
    *first = (uint32_t)(i < j ? i : j); *last = (uint32_t)(i < j ? j : i); *split = (uint32_t)g;
}
// the ref of the child that covers [first, last]: a leaf when it holds at most four keys, else internal node `index`
RT_LBVH_FN uint32_t lbvh_child_ref(uint32_t first, uint32_t last, uint32_t index)
{
    const uint32_t cnt = last - first + 1u;
    return cnt <= RT_LBVH_LEAF_TRIS ? lbvh_leafref(first, cnt) : index;
}
// the box of a leaf: over its slots in order, each slot's face being the low word of its key
RT_LBVH_FN void lbvh_leaf_box(uint32_t ref, const uint64_t *keys, const float *v, const uint32_t *f, float *box)
{
    const uint32_t first = ref & 0x0FFFFFFFu, cnt = ((ref >> 28) & 7u) + 1u;
    lbvh_box_empty(box);
    for (uint32_t k = 0; k < cnt; k++) lbvh_box_add_face(box, v, f + 3 * (uint64_t)(uint32_t)keys[first + k]);
}

// build_sah_bvh's area(): what the collapse orders the children by
RT_LBVH_FN float lbvh_area(const float *box)
{
    const float dx = box[3] - box[0], dy = box[4] - box[1], dz = box[5] - box[2];
    return 2.0f * (dx * dy + dy * dz + dz * dx);
}
// The four-wide collapse of binary node b (Col::go of rt_lower.cpp, not evenly): its two children, then, while there are fewer than
// four and an internal one is left, the internal child with the largest area (the first of equals) replaced by its own two, in
// place.  Returns the number of children; ref[] / box[] hold them (an internal ref is still a binary node's index here).
RT_LBVH_FN int lbvh_expand(const LbvhBin *bin, uint32_t b, uint32_t ref[4], float box[4][6])
{
    int n = 2;
    for (int i = 0; i < 2; i++) { ref[i] = bin[b].ref[i]; for (int k = 0; k < 6; k++) box[i][k] = bin[b].box[i][k]; }
    while (n < 4) {
        int pick = -1; float big = -1.0f;
        for (int i = 0; i < n; i++) if (!(ref[i] & RT_LBVH_LEAF)) { const float s = lbvh_area(box[i]); if (s > big) { big = s; pick = i; } }
        if (pick < 0) break;
        const uint32_t c = ref[pick];
        for (int i = n; i > pick + 1; i--) { ref[i] = ref[i - 1]; for (int k = 0; k < 6; k++) box[i][k] = box[i - 1][k]; }
        for (int i = 0; i < 2; i++) { ref[pick + i] = bin[c].ref[i]; for (int k = 0; k < 6; k++) box[pick + i][k] = bin[c].box[i][k]; }
        n++;
    }
    return n;
}
// the 128-byte record (32 words: float lo[3][4], hi[3][4], uint32 c[4], 16 bytes of zeros) of n children: the unused ones get NaN
// bounds and leafref(0, 1).  ref[] holds what the record is to hold (internal refs already record indices).
RT_LBVH_FN void lbvh_record(uint32_t *rec, int n, const uint32_t ref[4], const float box[4][6])
{
    for (int i = 0; i < 4; i++) {
        for (int a = 0; a < 3; a++) {
            float lo = __builtin_nanf(""), hi = __builtin_nanf("");
            if (i < n) { lo = box[i][a]; hi = box[i][3 + a]; }
            __builtin_memcpy(rec + 4 * a + i, &lo, 4);
            __builtin_memcpy(rec + 12 + 4 * a + i, &hi, 4);
        }
        rec[24 + i] = i < n ? ref[i] : lbvh_leafref(0u, 1u);
        rec[28 + i] = 0u;
    }
}

// ---- host only ---------------------------------------------------------------------------------------------------------
#include <string.h>

#include <algorithm>
#include <vector>

struct LbvhRecord { uint32_t w[32]; };   // one 128-byte node record (DevBvhNode of rt_dev.h)

// The tree rt_bvh_build.hip builds, from the functions of rt_lbvh.h it is made of, in plain loops: keys, std::sort, one pass over
// the internal nodes of the radix tree, the boxes child before parent, the collapse breadth-first through a queue.  No HIP call.
// level_off (may be NULL): where the records of every depth start (depth d is [level_off[d], level_off[d + 1])), the root's first.
inline void lbvh_build_host(const float *v, const uint32_t *f, size_t nf, std::vector<LbvhRecord> &out, std::vector<uint32_t> &slot_face,
                            uint32_t &root_ref, int &stack_need, std::vector<uint32_t> *level_off = nullptr)
{
    float cbox[6];
    lbvh_box_empty(cbox);
    for (size_t i = 0; i < nf; i++) {
        float c[3];
        lbvh_centroid(v, f + 3 * i, c);
        for (int a = 0; a < 3; a++) { cbox[a] = lbvh_min(cbox[a], c[a]); cbox[3 + a] = lbvh_max(cbox[3 + a], c[a]); }
    }
    std::vector<uint64_t> keys(nf);
    for (size_t i = 0; i < nf; i++) keys[i] = lbvh_key(v, f, (uint32_t)i, cbox);
    std::sort(keys.begin(), keys.end());
    slot_face.resize(nf);
    for (size_t i = 0; i < nf; i++) slot_face[i] = (uint32_t)keys[i];
    out.clear();
    stack_need = 0;
    if (level_off) level_off->assign(1, 0u);
    if (nf <= RT_LBVH_LEAF_TRIS) { root_ref = lbvh_leafref(0, (uint32_t)nf); return; }
    const size_t ni = nf - 1;
    std::vector<LbvhBin> bin(ni);
    std::vector<uint32_t> parent(ni, RT_LBVH_NO_PARENT);
    for (size_t i = 0; i < ni; i++) {
        uint32_t first, last, split;
        lbvh_range(keys.data(), (int64_t)nf, (int64_t)i, &first, &last, &split);
        if (last - first + 1u <= RT_LBVH_LEAF_TRIS) { bin[i].ref[0] = bin[i].ref[1] = RT_LBVH_DEAD; continue; }
        bin[i].ref[0] = lbvh_child_ref(first, split, split);
        bin[i].ref[1] = lbvh_child_ref(split + 1u, last, split + 1u);
        for (uint32_t side = 0; side < 2; side++) if (!(bin[i].ref[side] & RT_LBVH_LEAF)) parent[bin[i].ref[side]] = (uint32_t)(i << 1) | side;
    }
    // boxes: every node after its children, by an explicit stack from the root (the radix tree can be 60 levels deep)
    {
        std::vector<uint32_t> order, todo(1, 0u);
        while (!todo.empty()) {
            const uint32_t b = todo.back();
            todo.pop_back();
            order.push_back(b);
            for (int side = 0; side < 2; side++) if (!(bin[b].ref[side] & RT_LBVH_LEAF)) todo.push_back(bin[b].ref[side]);
        }
        for (size_t k = order.size(); k-- > 0; ) {
            const uint32_t b = order[k];
            for (int side = 0; side < 2; side++) {
                const uint32_t r = bin[b].ref[side];
                if (r & RT_LBVH_LEAF) lbvh_leaf_box(r, keys.data(), v, f, bin[b].box[side]);
                else { memcpy(bin[b].box[side], bin[r].box[0], 24); lbvh_box_add(bin[b].box[side], bin[r].box[1]); }
            }
        }
    }
    // the collapse, one depth after the other: the records of depth d + 1 follow those of depth d, by (parent record, child position)
    std::vector<uint32_t> rec_bin(1, 0u);
    std::vector<int> rec_held(1, 0);
    size_t off = 0;
    while (off < rec_bin.size()) {
        const size_t end = rec_bin.size();
        out.resize(end);
        for (size_t r = off; r < end; r++) {
            uint32_t ref[4]; float box[4][6];
            const int n = lbvh_expand(bin.data(), rec_bin[r], ref, box);
            const int held = rec_held[r] + n - 1;
            if (held > stack_need) stack_need = held;
            for (int i = 0; i < n; i++) if (!(ref[i] & RT_LBVH_LEAF)) { rec_bin.push_back(ref[i]); rec_held.push_back(held); ref[i] = (uint32_t)rec_bin.size() - 1u; }
            lbvh_record(out[r].w, n, ref, box);
        }
        off = end;
        if (level_off) level_off->push_back((uint32_t)end);
    }
    root_ref = 0;
}

#endif
