// rt_lower.cpp -- what puts a scene on a device: the lowering of the scene store (rt_api.cpp) to the device layout of rt_dev.h,
// the tree the kernels walk, in-place mesh updates.  prepare_device has rt_photons.cpp put the two photon maps beside it;
// rt_render.cpp renders from what it leaves; rt_host.h is what the host files share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/rt_mi355x.h"
#include "host/rt_scene.h"
#include "rt_host.h"
#include "rt_bvh_cost.h"
#include "rt_lbvh.h"
#include "rt_mesh_normals.h"

// ---- lowering to the device ---------------------------------------------------------------------------
static DeviceState *device_state(rt_scene *s, int device)
{
    for (DeviceState *d : s->devs) if (d->device == device) return d;
    DeviceState *d = new DeviceState;
    d->device = device;
    s->devs.push_back(d);
    return d;
}
// lookup only, under s->mu: NULL when nothing was ever prepared on that device (device_state above is the creating variant,
// for callers that hold s->mu)
DeviceState *find_device_state(rt_scene *s, int device)
{
    std::lock_guard<std::mutex> lk(s->mu);
    for (DeviceState *d : s->devs) if (d->device == device) return d;
    return nullptr;
}

// The tree the kernels walk is built HERE from the triangles (binned surface-area heuristic, leaves of at most four, collapsed
// four-wide by largest child first): any bounding hierarchy over the same triangles gives the same closest hit -- the
// triangle tests are the reference's, operation by operation, and `t < z` keeps the nearest whatever the order (only two
// hits at EXACTLY equal t depend on it) -- so the reference's mean-split tree (rt_bvh_build, rt_scene_set_mesh: kept bit-identical
// for whoever reads it back) is not what limits traversal any more.  slot_face: the face of every triangle slot (leaf order).
// stack_need: the most traversal-stack entries a ray can hold in this tree -- a visited node leaves (children - 1) entries behind
// while the ray is below it, so the maximum over root-to-leaf paths of the sum of (children - 1).  It never exceeds RT_BVH_LDS +
// RT_BVH_SPILL, what every tracing kernel provides: binned SAH over skewed geometry (sizes in geometric progression) peels one bin
// per binary level, far deeper than log2(n), and the collapse follows it down; when the tree does not fit it is built again with
// SAH splits only above a lower depth and balanced halves below (28, 26, .. 0).  The last resort, halves all the way, collapsed
// evenly (BOTH children replaced by theirs: every device level stands for two binary ones), always fits: halves over fewer
// than 2^28 faces with leaves of four are at most 26 binary levels deep, 13 device levels of at most 3 entries each.
// node_depth (may be NULL): the depth of every device node, the root's 0 -- what the refit orders its launches by.
static rt_status build_sah_bvh(const rt::MeshData &m, std::vector<DevBvhNode> &out, std::vector<uint32_t> &slot_face, uint32_t &root_ref, int &stack_need,
                               std::vector<uint32_t> *node_depth = nullptr)
{
    const size_t nf = m.f.size() / 3;
    struct TB { float lo[3], hi[3], c[3]; };
    std::vector<TB> tb(nf);
    for (size_t f = 0; f < nf; f++) {
        TB &t = tb[f];
        for (int a = 0; a < 3; a++) { t.lo[a] = 3.0e38f; t.hi[a] = -3.0e38f; }
        for (int k = 0; k < 3; k++) {
            const float *q = &m.v[3 * (size_t)m.f[3 * f + k]];
            for (int a = 0; a < 3; a++) { t.lo[a] = std::min(t.lo[a], q[a]); t.hi[a] = std::max(t.hi[a], q[a]); }
        }
        for (int a = 0; a < 3; a++) t.c[a] = 0.5f * (t.lo[a] + t.hi[a]);
    }
    if (nf >= 0x10000000ull) return fail(RT_ERR_LIMIT, "mesh too large");
    struct BN { float lo[3], hi[3]; int32_t left, right; uint32_t first, count; };      // binary tree: leaf when left < 0
    std::vector<BN> bn;
    std::vector<uint32_t> idx(nf);
    auto area = [](const float *lo, const float *hi) { const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2]; return 2.0f * (dx * dy + dy * dz + dz * dx); };
    struct Rec {
        std::vector<TB> &tb; std::vector<BN> &bn; std::vector<uint32_t> &idx; decltype(area) &area; int sah_depth;
        int32_t go(uint32_t b, uint32_t e, int depth)
        {
            BN n;
            for (int a = 0; a < 3; a++) { n.lo[a] = 3.0e38f; n.hi[a] = -3.0e38f; }
            float clo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, chi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
            for (uint32_t i = b; i < e; i++) {
                const TB &t = tb[idx[i]];
                for (int a = 0; a < 3; a++) { n.lo[a] = std::min(n.lo[a], t.lo[a]); n.hi[a] = std::max(n.hi[a], t.hi[a]); clo[a] = std::min(clo[a], t.c[a]); chi[a] = std::max(chi[a], t.c[a]); }
            }
            n.left = n.right = -1; n.first = b; n.count = e - b;
            const int32_t me = (int32_t)bn.size();
            bn.push_back(n);
            // leaves of at most four triangles (measured on MI355X, tracer ms Cornell / 102 k triangles / C3: 2: 15.45 / 21.77 / 202.4, 3: 15.46 / 21.79 /
            // 201.1, 4: 15.51 / 22.22 / 196.5, 6: 15.62 / 22.63 / 202.6, 8: 15.87 / 23.65 / 213.6), its triangles by face id
            if (e - b <= 4) { std::sort(idx.begin() + b, idx.begin() + e); return me; }
            uint32_t mid = 0;
            if (depth < sah_depth) {
                // binned SAH over the centroids, 16 bins per axis
                const int NB = 16;
                float best = 3.0e38f; int best_axis = -1, best_bin = 0;
                for (int a = 0; a < 3; a++) {
                    const float ext = chi[a] - clo[a];
                    if (!(ext > 0)) continue;
                    struct Bin { float lo[3], hi[3]; uint32_t n; } bins[NB];
                    for (int k = 0; k < NB; k++) { bins[k].n = 0; for (int c = 0; c < 3; c++) { bins[k].lo[c] = 3.0e38f; bins[k].hi[c] = -3.0e38f; } }
                    const float scale = (float)NB / ext;
                    for (uint32_t i = b; i < e; i++) {
                        const TB &t = tb[idx[i]];
                        int k = (int)((t.c[a] - clo[a]) * scale);
                        k = k < 0 ? 0 : (k >= NB ? NB - 1 : k);
                        bins[k].n++;
                        for (int c = 0; c < 3; c++) { bins[k].lo[c] = std::min(bins[k].lo[c], t.lo[c]); bins[k].hi[c] = std::max(bins[k].hi[c], t.hi[c]); }
                    }
                    float rlo[NB][3], rhi[NB][3]; uint32_t rn[NB];
                    float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f}; uint32_t cnt = 0;
                    for (int k = NB - 1; k >= 1; k--) {
                        cnt += bins[k].n;
                        for (int c = 0; c < 3; c++) { lo[c] = std::min(lo[c], bins[k].lo[c]); hi[c] = std::max(hi[c], bins[k].hi[c]); }
                        rn[k] = cnt; for (int c = 0; c < 3; c++) { rlo[k][c] = lo[c]; rhi[k][c] = hi[c]; }
                    }
                    for (int c = 0; c < 3; c++) { lo[c] = 3.0e38f; hi[c] = -3.0e38f; }
                    cnt = 0;
                    for (int k = 0; k + 1 < NB; k++) {               // split between bin k and k + 1
                        cnt += bins[k].n;
                        for (int c = 0; c < 3; c++) { lo[c] = std::min(lo[c], bins[k].lo[c]); hi[c] = std::max(hi[c], bins[k].hi[c]); }
                        if (cnt == 0 || rn[k + 1] == 0) continue;
                        const float cost = area(lo, hi) * (float)cnt + area(rlo[k + 1], rhi[k + 1]) * (float)rn[k + 1];
                        if (cost < best) { best = cost; best_axis = a; best_bin = k; }
                    }
                }
                if (best_axis >= 0) {
                    const int a = best_axis;
                    const float scale = 16.0f / (chi[a] - clo[a]);
                    auto it = std::partition(idx.begin() + b, idx.begin() + e, [&](uint32_t f) {
                        int k = (int)((tb[f].c[a] - clo[a]) * scale);
                        k = k < 0 ? 0 : (k >= 16 ? 15 : k);
                        return k <= best_bin;
                    });
                    mid = (uint32_t)(it - idx.begin());
                }
            }
            if (mid <= b || mid >= e) {
                // no usable plane (all centroids in one bin, or the tree got deep): halves by the widest centroid axis
                int a = 0;
                if (chi[1] - clo[1] > chi[a] - clo[a]) a = 1;
                if (chi[2] - clo[2] > chi[a] - clo[a]) a = 2;
                mid = b + (e - b) / 2;
                std::nth_element(idx.begin() + b, idx.begin() + mid, idx.begin() + e, [&](uint32_t x, uint32_t y) { return tb[x].c[a] < tb[y].c[a] || (tb[x].c[a] == tb[y].c[a] && x < y); });
            }
            const int32_t l = go(b, mid, depth + 1);
            const int32_t r = go(mid, e, depth + 1);
            bn[me].left = l; bn[me].right = r;
            return me;
        }
    };
    auto leafref = [](uint32_t off, uint32_t cnt) { return 0x80000000u | ((cnt - 1) << 28) | (off & 0x0FFFFFFFu); };
    // four-wide: a device node holds up to four descendants of the binary node it stands for -- starting from its two children, the
    // internal one with the largest surface is replaced by its own two children until there are four (or only leaves)
    // (evenly: both children replaced by theirs, see above.)  held: the stack entries of a ray that arrives at this node
    struct Col {
        std::vector<BN> &bn; std::vector<DevBvhNode> &out; decltype(area) &area; decltype(leafref) &leafref; bool evenly; int &need;
        std::vector<uint32_t> *node_depth;
        uint32_t go(int32_t id, int held, uint32_t depth)
        {
            const uint32_t me = (uint32_t)out.size();
            out.push_back(DevBvhNode{});
            if (node_depth) node_depth->push_back(depth);
            int32_t ch[4]; int n = 0;
            if (evenly) {
                for (const int32_t c : {bn[id].left, bn[id].right}) {
                    if (bn[c].left >= 0) { ch[n++] = bn[c].left; ch[n++] = bn[c].right; }
                    else ch[n++] = c;
                }
            } else { ch[n++] = bn[id].left; ch[n++] = bn[id].right; }
            while (!evenly && n < 4) {
                int pick = -1; float big = -1.0f;
                for (int i = 0; i < n; i++) if (bn[ch[i]].left >= 0) { const float s = area(bn[ch[i]].lo, bn[ch[i]].hi); if (s > big) { big = s; pick = i; } }
                if (pick < 0) break;
                const int32_t c = ch[pick];
                for (int i = n; i > pick + 1; i--) ch[i] = ch[i - 1];
                ch[pick] = bn[c].left; ch[pick + 1] = bn[c].right;
                n++;
            }
            held += n - 1;
            if (held > need) need = held;
            DevBvhNode d;
            memset(&d, 0, sizeof d);
            const float nan = std::nanf("");
            for (int i = 0; i < 4; i++) {
                for (int a = 0; a < 3; a++) { d.lo[a][i] = i < n ? bn[ch[i]].lo[a] : nan; d.hi[a][i] = i < n ? bn[ch[i]].hi[a] : nan; }
                if (i >= n) d.c[i] = leafref(0, 1);
                else if (bn[ch[i]].left < 0) d.c[i] = leafref(bn[ch[i]].first, bn[ch[i]].count);
                else d.c[i] = go(ch[i], held, depth + 1);
            }
            out[me] = d;
            return me;
        }
    };
    for (int sah_depth = 28; ; sah_depth -= 2) {
        bn.clear(); out.clear();
        if (node_depth) node_depth->clear();
        for (size_t i = 0; i < nf; i++) idx[i] = (uint32_t)i;
        Rec rec{tb, bn, idx, area, sah_depth};
        const int32_t root = rec.go(0, (uint32_t)nf, 0);
        stack_need = 0;
        Col col{bn, out, area, leafref, sah_depth == 0, stack_need, node_depth};
        if (bn[root].left < 0) root_ref = leafref(bn[root].first, bn[root].count);
        else root_ref = col.go(root, 0, 0);
        if (stack_need <= RT_BVH_LDS + RT_BVH_SPILL) break;
        if (sah_depth == 0) return fail(RT_ERR_LIMIT, "the BVH can need %d traversal-stack entries, the device provides %d", stack_need, RT_BVH_LDS + RT_BVH_SPILL);      // not reached: see above
    }
    slot_face = idx;
    return RT_OK;
}

// the tree of one mesh as upload_scene would build it, for whoever wants to look at it on the host (no device, no HIP call)
extern "C" rt_status rt_scene_mesh_device_bvh(const rt_scene *s, int32_t mesh, rt_device_bvh_info *info, void *nodes, uint64_t nodes_cap,
                                              uint32_t *slot_face, uint64_t slots_cap)
{
    if (!s || !info) return fail(RT_ERR_ARG, "rt_scene_mesh_device_bvh: NULL argument");
    if (info->struct_size != sizeof(rt_device_bvh_info))
        return fail(RT_ERR_ARG, "rt_scene_mesh_device_bvh: rt_device_bvh_info.struct_size is %u, this library's is %zu", info->struct_size, sizeof(rt_device_bvh_info));
    std::vector<DevBvhNode> bn;
    std::vector<uint32_t> faces;
    uint32_t root_ref = 0;
    int need = 0;
    {
        std::lock_guard<std::mutex> lk(const_cast<rt_scene *>(s)->mu);
        if (mesh < 0 || (size_t)mesh >= s->data.meshes.size() || s->data.meshes[mesh].f.empty()) return fail(RT_ERR_ARG, "rt_scene_mesh_device_bvh: mesh %d was never set", mesh);
        rt_status st = build_sah_bvh(s->data.meshes[mesh], bn, faces, root_ref, need);
        if (st) return st;
    }
    // both capacities before anything is written: a refused call leaves info and both buffers as they were
    if (nodes && nodes_cap < bn.size()) return fail(RT_ERR_ARG, "rt_scene_mesh_device_bvh: room for %llu node records, %zu needed", (unsigned long long)nodes_cap, bn.size());
    if (slot_face && slots_cap < faces.size()) return fail(RT_ERR_ARG, "rt_scene_mesh_device_bvh: room for %llu triangle slots, %zu needed", (unsigned long long)slots_cap, faces.size());
    info->n_nodes = (uint32_t)bn.size(); info->n_slots = (uint32_t)faces.size();
    info->root_ref = root_ref; info->stack_need = need;
    info->bvh_lds = RT_BVH_LDS; info->bvh_stack = RT_BVH_STACK; info->bvh_spill = RT_BVH_SPILL;
    info->spill_blocks = RT_SPILL_BLOCKS; info->block = RT_BLOCK;
    if (nodes) memcpy(nodes, bn.data(), bn.size() * sizeof(DevBvhNode));
    if (slot_face) memcpy(slot_face, faces.data(), faces.size() * 4);
    return RT_OK;
}

// ---- device tree build: the host mirror (rt_mi355x.h, "device tree build") ----------------------------------------------------
// lbvh_build_host of rt_lbvh.h, the functions the kernels of rt_bvh_build.hip are made of in plain loops, behind the ABI's argument checks
extern "C" rt_status rt_device_lbvh_build(const float *v, int32_t nv, const uint32_t *f, int32_t nf, rt_device_bvh_info *info, void *nodes,
                                          uint64_t nodes_cap, uint32_t *slot_face, uint64_t slots_cap)
{
    if (!v || !f || !info) return fail(RT_ERR_ARG, "rt_device_lbvh_build: NULL argument");
    if (info->struct_size != sizeof(rt_device_bvh_info))
        return fail(RT_ERR_ARG, "rt_device_lbvh_build: rt_device_bvh_info.struct_size is %u, this library's is %zu", info->struct_size, sizeof(rt_device_bvh_info));
    if (nv <= 0 || nf <= 0) return fail(RT_ERR_ARG, "rt_device_lbvh_build: nv is %d and nf is %d (both must be positive)", nv, nf);
    if ((uint32_t)nf >= 0x10000000u) return fail(RT_ERR_LIMIT, "mesh too large");
    for (int64_t i = 0; i < 3LL * nf; i++) if (f[i] >= (uint32_t)nv) return fail(RT_ERR_ARG, "rt_device_lbvh_build: face index %u >= nv", f[i]);
    std::vector<LbvhRecord> bn;
    std::vector<uint32_t> faces;
    uint32_t root_ref = 0;
    int need = 0;
    lbvh_build_host(v, f, (size_t)nf, bn, faces, root_ref, need);
    // both capacities before anything is written: a refused call leaves info and both buffers as they were
    if (nodes && nodes_cap < bn.size()) return fail(RT_ERR_ARG, "rt_device_lbvh_build: room for %llu node records, %zu needed", (unsigned long long)nodes_cap, bn.size());
    if (slot_face && slots_cap < faces.size()) return fail(RT_ERR_ARG, "rt_device_lbvh_build: room for %llu triangle slots, %zu needed", (unsigned long long)slots_cap, faces.size());
    info->n_nodes = (uint32_t)bn.size(); info->n_slots = (uint32_t)faces.size();
    info->root_ref = root_ref; info->stack_need = need;
    info->bvh_lds = RT_BVH_LDS; info->bvh_stack = RT_BVH_STACK; info->bvh_spill = RT_BVH_SPILL;
    info->spill_blocks = RT_SPILL_BLOCKS; info->block = RT_BLOCK;
    if (nodes && !bn.empty()) memcpy(nodes, bn.data(), bn.size() * sizeof(DevBvhNode));
    if (slot_face) memcpy(slot_face, faces.data(), faces.size() * 4);
    return RT_OK;
}

// The class word of a material (RT_MAT_*, rt_dev.h): decided here, once per material, so that shade_fin can leave out arithmetic
// whose result is exactly +0 for EVERY hit on that material.  Bit patterns are compared, not values: -0.0f and NaN keep the
// general path (a -0 weight changes the sign of a zero sum, a NaN must reach the pixel).
//   RT_MAT_NO_SPEC_TREE: reflection and refraction are +0 in all channels (they are plain colours in rt_blinn: no texture map can
//     scale them) and ior is finite and > 0.  Shade's rK / tK are then (+0) + (+0) * rC and (+0) * tC (FIN/main.cpp:601-610); rC is
//     finite for a finite ray when ior > 0 (eta and C0 are finite, powf(1 - |cosI|, 5) lies in [0, 1]), so both are zeros,
//     neither exceeds the 0.001 threshold, no child ray exists and nobody reads the two directions.  (A NaN weight would fail
//     the threshold test the same way.)
//   RT_MAT_NO_SPECULAR: ks is +0 in all channels, the specular colour has no texture map, glossiness is finite and in [0, 2^20].
//     The lobe is powf(cosNH, gloss) with cosNH = max(0, N.H) of two unit vectors: in [0, 1] up to the rounding of two
//     normalisations and a dot product (1 + 1e-6 at the very most), so the power is finite and >= 0 -- [0, 1] for cosNH <= 1,
//     below exp(2^20 * 1e-6) < 3 beyond; 0^0 = 1 -- and (ks * intensity) * power has the bits of ks * intensity, a zero or, for
//     a non-finite intensity, a NaN.  The upper bound on glossiness is what keeps the power from overflowing to +inf (0 * inf = NaN).
static uint32_t material_class_of(const rt_blinn &m, const rt_texmap *maps)
{
    auto pos_zero3 = [](const float *c) { uint32_t b[3]; memcpy(b, c, 12); return (b[0] | b[1] | b[2]) == 0u; };
    uint32_t cls = 0;
    if (pos_zero3(m.reflection) && pos_zero3(m.refraction) && std::isfinite(m.ior) && m.ior > 0.0f) cls |= RT_MAT_NO_SPEC_TREE;
    const bool spec_map = maps && maps[1].texture != RT_MAP_NONE;
    if (pos_zero3(m.specular) && !spec_map && std::isfinite(m.glossiness) && m.glossiness >= 0.0f && m.glossiness <= 1048576.0f) cls |= RT_MAT_NO_SPECULAR;
    return cls;
}
// one word per material as upload_scene puts it on a device; all clear under RT_RENDER_GENERAL_SHADING (caller holds s->mu)
static void lower_material_classes(const rt_scene *s, std::vector<uint32_t> &out)
{
    const rt::SceneData &sd = s->data;
    const bool general = (s->render_flags.load() & RT_RENDER_GENERAL_SHADING) != 0;
    const bool mapped = sd.material_maps.size() == 2 * sd.materials.size();
    out.assign(sd.materials.size(), 0u);
    if (!general) for (size_t i = 0; i < sd.materials.size(); i++) out[i] = material_class_of(sd.materials[i], mapped ? &sd.material_maps[2 * i] : nullptr);
}
// the class words as upload_scene would set them, for whoever wants to look at them on the host (no device, no HIP call)
extern "C" rt_status rt_scene_material_classes(const rt_scene *s, uint32_t *out, int32_t cap, int32_t *n_out)
{
    if (!s || (!out && cap > 0)) return fail(RT_ERR_ARG, "rt_scene_material_classes: NULL argument");
    std::vector<uint32_t> cls;
    {
        std::lock_guard<std::mutex> lk(const_cast<rt_scene *>(s)->mu);
        lower_material_classes(s, cls);
    }
    if (n_out) *n_out = (int32_t)cls.size();
    if (cap < 0 || (out && (size_t)cap < cls.size())) return fail(RT_ERR_ARG, "rt_scene_material_classes: room for %d words, %zu needed", cap, cls.size());
    if (out && !cls.empty()) memcpy(out, cls.data(), cls.size() * 4);
    return RT_OK;
}

static DevNodeXf xf_of(const rt_node &n)
{
    DevNodeXf x;
    memcpy(x.itm, n.itm, 36); memcpy(x.pos, n.pos, 12); memcpy(x.tm, n.tm, 36);
    x.pad[0] = x.pad[1] = x.pad[2] = 0;
    return x;
}

// the local extent of a mesh, lo[3] hi[3]: the root box of its cyBVH arrays (of the ones a vertex update will have built again)
static const float *mesh_root_box(const rt::MeshData &m) { return m.tree_stale ? m.root_box : m.nodes[1].box; }

// The DevObject / DevObjectBack records of the scene's objects and the material of every node: shared by upload_scene and by the
// in-place mesh update (refit_mesh_on_devices), which moves the cull boxes of the objects whose mesh changed.
static rt_status lower_objects(const rt::SceneData &sd, std::vector<DevObject> &objs, std::vector<DevObjectBack> &backs, std::vector<int32_t> &node_mat)
{
    const int nn = (int)sd.nodes.size();
    objs.clear(); backs.clear();
    node_mat.assign(nn, 0);
    // The objects are emitted in the order TraceNode visits them (FIN/main.cpp:108-130): depth-first from node 0, a node's own
    // object first, then its children by ascending index -- NOT in the order of the array, which only has to put parents before
    // children.  The order shows in the results: every comparison of the object loop is strict, so of two objects at exactly
    // the same distance the first one tested wins, and a FIN mesh hit keeps the uvw of the sphere / plane hit accepted before
    // it.  (An array in depth-first pre-order, like every array the XML loader makes, is visited in index order.)
    std::vector<int> visit;
    {
        std::vector<int> first_child(nn, -1), last_child(nn, -1), next_sibling(nn, -1);
        for (int i = 1; i < nn; i++) {                                       // ascending i: the sibling lists come out ascending
            const int p = sd.nodes[i].parent;                                 // 0 <= p < i: rt_scene_set_nodes checked it
            if (last_child[p] < 0) first_child[p] = i; else next_sibling[last_child[p]] = i;
            last_child[p] = i;
        }
        visit.reserve(nn);
        for (int i = 0; i >= 0; ) {
            visit.push_back(i);
            if (first_child[i] >= 0) { i = first_child[i]; continue; }
            while (i >= 0 && next_sibling[i] < 0) i = sd.nodes[i].parent;     // up to the nearest ancestor with a sibling left
            if (i >= 0) i = next_sibling[i];
        }
    }
    for (const int i : visit) {
        const rt_node &n = sd.nodes[i];
        if (n.obj_type == RT_OBJ_NONE) continue;
        if (n.material < 0 || (size_t)n.material >= sd.materials.size())
            return fail(RT_ERR_ARG, "node %d carries an object but its material index %d is invalid", i, n.material);
        node_mat[i] = n.material;
        DevObject o{};
        o.type = n.obj_type; o.mesh = -1; o.material = n.material; o.node = i;
        if (n.obj_type == RT_OBJ_MESH) {
            if (n.mesh < 0 || (size_t)n.mesh >= sd.meshes.size() || sd.meshes[n.mesh].f.empty())
                return fail(RT_ERR_ARG, "node %d references mesh %d which was never set", i, n.mesh);
            o.mesh = n.mesh;
        }
        int chain[64], len = 0;
        for (int a = i; a >= 0; a = sd.nodes[a].parent) { if (len >= 64) break; chain[len++] = a; }
        if (len > RT_MAX_DEPTH) return fail(RT_ERR_LIMIT, "node %d is nested %d deep; the device supports %d levels", i, len, RT_MAX_DEPTH);
        o.chain_len = len;
        for (int c = 0; c < len; c++) o.chain[c] = chain[len - 1 - c];      // root .. self
        memcpy(o.own_itm, n.itm, 36); memcpy(o.own_pos, n.pos, 12);         // the node's own ToNodeCoords transform, beside the rest
        {   // bounds in the ROOT node's coordinates (where every ray is taken first): the 8 corners of the
            // local extent through tm*p + pos of self .. the root's child (double), inflated by 1e-3 of
            // the extent (the exact test runs in float in local space)
            double lo[3] = {-1, -1, -1}, hi[3] = {1, 1, 1};                 // unit sphere; unit square at z = 0
            if (n.obj_type == RT_OBJ_PLANE) lo[2] = hi[2] = 0;
            if (n.obj_type == RT_OBJ_MESH) {
                const float *b = mesh_root_box(sd.meshes[n.mesh]);
                for (int a = 0; a < 3; a++) { lo[a] = b[a]; hi[a] = b[a + 3]; }
            }
            double wlo[3] = {1e300, 1e300, 1e300}, whi[3] = {-1e300, -1e300, -1e300};
            bool finite = true;
            for (int corner = 0; corner < 8; corner++) {
                double q[3] = {(corner & 1) ? hi[0] : lo[0], (corner & 2) ? hi[1] : lo[1], (corner & 4) ? hi[2] : lo[2]};
                for (int c = 0; c + 1 < len; c++) {                          // chain[] here is still self .. root
                    const rt_node &X = sd.nodes[chain[c]];
                    const double r[3] = {q[0] * X.tm[0] + q[1] * X.tm[3] + q[2] * X.tm[6] + X.pos[0],
                                         q[0] * X.tm[1] + q[1] * X.tm[4] + q[2] * X.tm[7] + X.pos[1],
                                         q[0] * X.tm[2] + q[1] * X.tm[5] + q[2] * X.tm[8] + X.pos[2]};
                    q[0] = r[0]; q[1] = r[1]; q[2] = r[2];
                }
                for (int a = 0; a < 3; a++) { if (!std::isfinite(q[a])) finite = false; wlo[a] = std::min(wlo[a], q[a]); whi[a] = std::max(whi[a], q[a]); }
            }
            const double ext = std::max(std::max(whi[0] - wlo[0], whi[1] - wlo[1]), whi[2] - wlo[2]);
            const double pad = 1e-3 * ext + 1e-5;
            for (int a = 0; a < 3; a++) {
                // a degenerate transform (non-finite corner) disables the cull for this object
                o.wlo[a] = finite ? (float)(wlo[a] - pad) : -3.0e38f;
                o.whi[a] = finite ? (float)(whi[a] + pad) : 3.0e38f;
            }
        }
        objs.push_back(o);
        DevObjectBack b;
        memset(&b, 0, sizeof b);
        b.chain_len = len; b.node = i;
        for (int k = 0; k < RT_BACK_LEVELS && k < len - 1; k++) b.lvl[k] = xf_of(sd.nodes[chain[k]]);     // chain[] is self .. root
        backs.push_back(b);
    }
    if (objs.size() > RT_MAX_OBJECTS) return fail(RT_ERR_LIMIT, "too many objects (%zu)", objs.size());
    return RT_OK;
}

static rt_status upload_scene(rt_scene *s, DeviceState *D)
{
    const rt::SceneData &sd = s->data;
    if (sd.nodes.empty()) return fail(RT_ERR_STATE, "scene has no nodes");
    if (sd.nodes.size() > 65535) return fail(RT_ERR_LIMIT, "too many scene nodes (%zu)", sd.nodes.size());
    if (sd.materials.size() > 65535) return fail(RT_ERR_LIMIT, "too many materials (%zu): ray records carry 16-bit material indices", sd.materials.size());
    const int nn = (int)sd.nodes.size();
    std::vector<DevNodeXf> xf(nn);
    std::vector<int32_t> node_mat;
    std::vector<DevObject> objs;
    std::vector<DevObjectBack> backs;
    for (int i = 0; i < nn; i++) xf[i] = xf_of(sd.nodes[i]);
    rt_status st;
    if ((st = lower_objects(sd, objs, backs, node_mat))) return st;
    if ((st = D->nodes.upload(xf.data(), xf.size() * sizeof(DevNodeXf)))) return st;
    if ((st = D->objects.upload(objs.data(), objs.size() * sizeof(DevObject)))) return st;
    if ((st = D->objects_back.upload(backs.data(), backs.size() * sizeof(DevObjectBack)))) return st;
    if ((st = D->node_material.upload(node_mat.data(), node_mat.size() * 4))) return st;
    D->node_object.assign((size_t)nn, -1);
    for (size_t k = 0; k < objs.size(); k++) D->node_object[objs[k].node] = (int32_t)k;
    if ((st = D->materials.upload(sd.materials.data(), sd.materials.size() * sizeof(rt_blinn)))) return st;
    std::vector<uint32_t> mat_class;
    lower_material_classes(s, mat_class);
    if ((st = D->material_class.upload(mat_class.data(), mat_class.size() * 4))) return st;
    if ((st = D->lights.upload(sd.lights.data(), sd.lights.size() * sizeof(rt_light)))) return st;

    for (auto &mb : D->mesh_bufs) mb.release();
    D->mesh_bufs.assign(sd.meshes.size(), DevMeshBufs());
    std::vector<DevMesh> dm(sd.meshes.size());
    int max_depth = 0;
    for (size_t mi = 0; mi < sd.meshes.size(); mi++) {
        ensure_normals(s->data.meshes[mi]);      // SMOOTH mode: the normals of the v of now, which a device updated in place holds already
        const rt::MeshData &m = sd.meshes[mi];
        memset(&dm[mi], 0, sizeof(DevMesh));
        if (m.f.empty()) continue;
        std::vector<DevBvhNode> bn;
        uint32_t root_ref = 0;
        int depth = 0;
        std::vector<uint32_t> slot_face, node_depth;
        if ((st = build_sah_bvh(m, bn, slot_face, root_ref, depth, &node_depth))) return st;
        // (the smallest LDS stack of any tracing kernel is RT_BVH_LDS entries; RT_BVH_SPILL more per thread wait in HBM: spill buffers
        // below.  The builder keeps every tree within that: this only guards the kernels against a builder that does not.)
        if (depth > RT_BVH_LDS + RT_BVH_SPILL) return fail(RT_ERR_LIMIT, "mesh %zu: the BVH can need %d traversal-stack entries, the device provides %d", mi, depth, RT_BVH_LDS + RT_BVH_SPILL);
        max_depth = std::max(max_depth, depth);
        const size_t nf = m.f.size() / 3;
        std::vector<DevTri> tris(nf);
        std::vector<uint32_t> tri_face(nf);
        std::vector<float> nrm(9 * nf);
        for (size_t sidx = 0; sidx < nf; sidx++) {
            const uint32_t face = slot_face[sidx];
            tri_face[sidx] = face;
            rt::Point3 P[3];
            for (int k = 0; k < 3; k++) { const float *q = &m.v[3 * (size_t)m.f[3 * (size_t)face + k]]; P[k] = rt::Point3(q[0], q[1], q[2]); }
            rt::Point3 N = (P[1] - P[0]).Cross(P[2] - P[0]);      // FIN/include/objects.h:234-235
            N.Normalize();
            DevTri &T = tris[sidx];
            T.A[0] = P[0].x; T.A[1] = P[0].y; T.A[2] = P[0].z; T.B[0] = P[1].x; T.B[1] = P[1].y; T.B[2] = P[1].z;
            T.C[0] = P[2].x; T.C[1] = P[2].y; T.C[2] = P[2].z; T.N[0] = N.x; T.N[1] = N.y; T.N[2] = N.z;
        }
        for (size_t sidx = 0; sidx < nf; sidx++)                 // per triangle SLOT (leaf order), like tris
            for (int k = 0; k < 3; k++) memcpy(&nrm[9 * sidx + 3 * k], &m.vn[3 * (size_t)m.fn[3 * (size_t)tri_face[sidx] + k]], 12);
        DevMeshBufs &mb = D->mesh_bufs[mi];
        if ((st = mb.nodes.upload(bn.data(), bn.size() * sizeof(DevBvhNode)))) return st;
        if ((st = mb.tris.upload(tris.data(), tris.size() * sizeof(DevTri)))) return st;
        if ((st = mb.nrm.upload(nrm.data(), nrm.size() * 4))) return st;
        if (!m.v_prev.empty() && (st = mb.v_prev.upload(m.v_prev.data(), m.v_prev.size() * 4))) return st;      // survives a rebuild: per vertex, not per slot
        {   // what an in-place vertex update works from (DevMeshBufs): the slots' indices, and the nodes by depth, deepest first
            std::vector<uint32_t> slot_idx(6 * nf);
            for (size_t sidx = 0; sidx < nf; sidx++)
                for (int k = 0; k < 3; k++) { slot_idx[6 * sidx + k] = m.f[3 * (size_t)tri_face[sidx] + k]; slot_idx[6 * sidx + 3 + k] = m.fn[3 * (size_t)tri_face[sidx] + k]; }
            uint32_t levels = 0;
            for (const uint32_t d : node_depth) levels = std::max(levels, d + 1);
            mb.level_off.assign((size_t)levels + 1, 0);
            for (const uint32_t d : node_depth) mb.level_off[levels - d]++;                   // level k = depth levels - 1 - k: counts at [k + 1]
            for (uint32_t k = 0; k < levels; k++) mb.level_off[k + 1] += mb.level_off[k];
            std::vector<uint32_t> level_nodes(node_depth.size()), at(mb.level_off.begin(), mb.level_off.end() - 1);
            for (size_t i = 0; i < node_depth.size(); i++) level_nodes[at[levels - 1 - node_depth[i]]++] = (uint32_t)i;
            if ((st = mb.slot_idx.upload(slot_idx.data(), slot_idx.size() * 4))) return st;
            if ((st = mb.level_nodes.upload(level_nodes.data(), level_nodes.size() * 4))) return st;
            mb.slot_face = tri_face; mb.root_ref = root_ref; mb.stack_need = depth;
            bvh_cost_host(bn.data(), bn.size(), root_ref, &mb.built_cost, &mb.built_flags);      // (root_ref is the builder's own: always there)
        }
        dm[mi].tex = nullptr;
        if (!m.vt.empty() && m.ft.size() == m.f.size()) {      // vt[ft0], vt[ft1], vt[ft2] per triangle slot, like nrm
            std::vector<float> tex(9 * nf);
            for (size_t sidx = 0; sidx < nf; sidx++)
                for (int k = 0; k < 3; k++) memcpy(&tex[9 * sidx + 3 * k], &m.vt[3 * (size_t)m.ft[3 * (size_t)tri_face[sidx] + k]], 12);
            if ((st = mb.tex.upload(tex.data(), tex.size() * 4))) return st;
            dm[mi].tex = (const float *)mb.tex.p;
        }
        dm[mi].nodes = (const DevBvhNode *)mb.nodes.p; dm[mi].tris = (const DevTri *)mb.tris.p;
        dm[mi].nrm = (const float *)mb.nrm.p;
        memcpy(dm[mi].root_box, mesh_root_box(m), 24);
        dm[mi].root_ref = root_ref; dm[mi].n_tris = (uint32_t)nf;
    }
    if ((st = D->meshes.upload(dm.data(), dm.size() * sizeof(DevMesh)))) return st;

    DevScene &S = D->scene;
    S.nodes = (const DevNodeXf *)D->nodes.p; S.objects = (const DevObject *)D->objects.p; S.objects_back = (const DevObjectBack *)D->objects_back.p;
    S.meshes = (const DevMesh *)D->meshes.p; S.materials = (const rt_blinn *)D->materials.p; S.material_class = (const uint32_t *)D->material_class.p;
    S.lights = (const rt_light *)D->lights.p; S.node_material = (const int32_t *)D->node_material.p;
    S.n_nodes = nn; S.n_objects = (int)objs.size(); S.n_meshes = (int)sd.meshes.size();
    S.n_materials = (int)sd.materials.size(); S.n_lights = (int)sd.lights.size();
    memcpy(S.env, sd.env, 12); memcpy(S.bg, sd.bg, 12);
    // textures and maps
    for (const rt_texture &t : sd.textures)
        if (t.type == RT_TEX_FILE && (t.width < 0 || t.height < 0 || (uint64_t)t.texel_offset + 3ull * t.width * t.height > sd.texels.size()))
            return fail(RT_ERR_ARG, "texture texels out of range");
    if (!sd.material_maps.empty() && sd.material_maps.size() != 2 * sd.materials.size())
        return fail(RT_ERR_ARG, "material maps: need 2 per material (%zu given for %zu materials)", sd.material_maps.size(), sd.materials.size());
    auto check_map = [&](const rt_texmap &m) { return m.texture == RT_MAP_NONE || m.texture == RT_MAP_EMPTY || (m.texture >= 0 && (size_t)m.texture < sd.textures.size()); };
    for (const rt_texmap &m : sd.material_maps) if (!check_map(m)) return fail(RT_ERR_ARG, "material map refers to texture %d", m.texture);
    if (!check_map(sd.env_map) || !check_map(sd.bg_map)) return fail(RT_ERR_ARG, "environment/background map refers to a missing texture");
    if ((st = D->textures.upload(sd.textures.data(), sd.textures.size() * sizeof(rt_texture)))) return st;
    if ((st = D->texels.upload(sd.texels.data(), sd.texels.size()))) return st;
    if ((st = D->material_maps.upload(sd.material_maps.data(), sd.material_maps.size() * sizeof(rt_texmap)))) return st;
    S.textures = (const rt_texture *)D->textures.p; S.texels = (const uint8_t *)D->texels.p; S.n_textures = (int)sd.textures.size();
    S.material_maps = sd.material_maps.empty() ? nullptr : (const rt_texmap *)D->material_maps.p;
    S.env_map = sd.env_map; S.bg_map = sd.bg_map;
    S.use_uvw = sd.material_maps.empty() ? 0 : 1;
    S.max_bvh_depth = max_depth;
    S.bvh_spill = nullptr;
    if (max_depth > RT_BVH_LDS) {
        if ((st = D->bvh_spill.ensure(SPILL_BYTES))) return st;
        S.bvh_spill = (uint32_t *)D->bvh_spill.p;
    }
    S.stochastic = 0;
    for (const rt_light &l : sd.lights) if (l.type == RT_LIGHT_POINT && l.size != 0) S.stochastic = 1;
    for (const rt_blinn &m : sd.materials) if (m.reflection_glossiness != 0 || m.refraction_glossiness != 0) S.stochastic = 1;
    D->scene_valid = true;
    return RT_OK;
}

// ---- mesh vertex updates -------------------------------------------------------------------------------
// One device's share of rt_scene_update_mesh_vertices: everything upload_scene derived from this mesh's vertices, set again in
// place -- DevTri and nrm of every slot and every box of the tree (rt_refit.hip), DevMesh::root_box, and the objects' cull boxes
// (objs: the scene's objects lowered again by the caller).  Nothing else on the device depends on a mesh's vertices: the tree's
// topology, stack_need (DevScene::max_bvh_depth, the spill buffers) and tex follow the faces, which stay.
static rt_status enqueue_mesh_cost(DeviceState *D, DevMeshBufs &mb);
static rt_status finish_mesh_cost(DeviceState *D, const DevMeshBufs &mb, rt_mesh_quality *q);

// Smooth normals (rt_mi355x.h, "smooth normals"), one device's share in two steps.  prepare: what k_mesh_normals works from, on
// the device from the mesh's first update in SMOOTH mode there -- the adjacency over normal indices, built here by a counting
// sort that follows the faces, and the face indices (which a device build may have brought already).  enqueue: the launch on the
// update's stream, behind the vertex upload and ahead of k_mesh_retri, between the events rt_scene_mesh_normals_ms reads.
static rt_status prepare_mesh_normals(DeviceState *D, const rt::MeshData &m, DevMeshBufs &mb)
{
    rt_status rs;
    for (Event &e : D->nrm_ev) if (!e.e) HIP_TRY(e.create());
    if (!mb.f.p && (rs = mb.f.upload(m.f.data(), m.f.size() * 4))) return rs;
    if (mb.nadj_off.p && mb.nadj_corner.p) return RT_OK;
    const size_t nvn = m.vn.size() / 3;
    std::vector<uint32_t> off(nvn + 1), corner(m.fn.size());
    mesh_normal_adjacency(m.fn.data(), m.fn.size() / 3, nvn, off.data(), corner.data());
    if ((rs = mb.nadj_corner.upload(corner.data(), corner.size() * 4))) return rs;
    return mb.nadj_off.upload(off.data(), off.size() * 4);
}
static rt_status enqueue_mesh_normals(DeviceState *D, const rt::MeshData &m, DevMeshBufs &mb)
{
    MeshNormalsRequest N = {};
    N.v = (const float *)mb.v.p; N.f = (const uint32_t *)mb.f.p;
    N.nadj_off = (const uint32_t *)mb.nadj_off.p; N.nadj_corner = (const uint32_t *)mb.nadj_corner.p;
    N.n_normals = (uint32_t)(m.vn.size() / 3); N.vn = (float *)mb.vn.p;
    HIP_TRY(hipEventRecord(D->nrm_ev[0], D->stream));
    HIP_TRY(rtk_launch_mesh_normals(D->stream, N));
    HIP_TRY(hipEventRecord(D->nrm_ev[1], D->stream));
    D->nrm_timed = true;
    return RT_OK;
}

static rt_status refit_mesh_on_device(DeviceState *D, rt::MeshData &m, int32_t mesh, bool normals_changed, const std::vector<DevObject> &objs,
                                      rt_mesh_quality *quality)
{
    HIP_TRY(hipSetDevice(D->device));
    if (D->last_pending && D->last_done) HIP_TRY(hipEventSynchronize(D->last_done));      // an asynchronous render may still be tracing this mesh
    rt_status rs;
    if ((rs = motion_wait_host(D->device))) return rs;                                      // ... or k_motion_mesh walking it
    const size_t nf = m.f.size() / 3;
    if ((size_t)mesh >= D->mesh_bufs.size() || D->mesh_bufs[mesh].slot_face.size() != nf || objs.size() != (size_t)D->scene.n_objects)
        return fail(RT_ERR_STATE, "rt_scene_update_mesh_vertices: device %d does not hold mesh %d as the scene has it", D->device, mesh);
    DevMeshBufs &mb = D->mesh_bufs[mesh];
    hipStream_t st = D->stream;
    for (Event &e : D->upd_ev) if (!e.e) HIP_TRY(e.create());
    const bool first = mb.vn.p == nullptr;
    // SMOOTH mode and no normals brought: the device computes them from the vertices it is about to be sent
    const bool smooth = m.normals_mode == RT_MESH_NORMALS_SMOOTH && !normals_changed;
    if ((rs = mb.v.ensure(m.v.size() * 4)) || (rs = mb.vn.ensure(m.vn.size() * 4))) return rs;
    if (smooth && (rs = prepare_mesh_normals(D, m, mb))) return rs;
    // the store's normals are about to be read: never stale ones over what k_mesh_normals wrote here (the first time they are
    // the values the kernel's kept normals keep)
    if (first || normals_changed) ensure_normals(m);
    // the previous positions follow the store: uploaded from it ahead of the new vertices, in the update's stream, by a flagged
    // update; released by an unflagged one (nothing is allocated, copied or freed for a mesh that never used the flag)
    if (m.v_prev.empty()) mb.v_prev.release();
    else if ((rs = mb.v_prev.ensure(m.v_prev.size() * 4))) return rs;
    HIP_TRY(hipEventRecord(D->upd_ev[0], st));
    if (!m.v_prev.empty()) HIP_TRY(hipMemcpyAsync(mb.v_prev.p, m.v_prev.data(), m.v_prev.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(mb.v.p, m.v.data(), m.v.size() * 4, hipMemcpyHostToDevice, st));
    if (first || normals_changed) HIP_TRY(hipMemcpyAsync(mb.vn.p, m.vn.data(), m.vn.size() * 4, hipMemcpyHostToDevice, st));
    if (smooth && (rs = enqueue_mesh_normals(D, m, mb))) return rs;
    HIP_TRY(hipEventRecord(D->upd_ev[1], st));
    MeshRefitRequest R = {};
    R.v = (const float *)mb.v.p; R.vn = (const float *)mb.vn.p;
    R.slot_idx = (const uint32_t *)mb.slot_idx.p; R.n_slots = (uint32_t)nf;
    R.tris = (DevTri *)mb.tris.p; R.nrm = (float *)mb.nrm.p; R.nodes = (DevBvhNode *)mb.nodes.p;
    R.level_nodes = (const uint32_t *)mb.level_nodes.p; R.level_off = mb.level_off.data(); R.n_levels = (int)mb.level_off.size() - 1;
    R.after_retri = D->upd_ev[2];
    HIP_TRY(rtk_launch_mesh_refit(st, R));
    HIP_TRY(hipEventRecord(D->upd_ev[3], st));
    D->upd_levels = R.n_levels;
    HIP_TRY(hipMemcpyAsync((char *)D->meshes.p + (size_t)mesh * sizeof(DevMesh) + offsetof(DevMesh, root_box), m.root_box, 24, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(D->objects.p, objs.data(), objs.size() * sizeof(DevObject), hipMemcpyHostToDevice, st));
    if (quality && (rs = enqueue_mesh_cost(D, mb))) return rs;      // the refitted tree, measured behind the refit on the same stream
    HIP_TRY(hipStreamSynchronize(st));
    return quality ? finish_mesh_cost(D, mb, quality) : RT_OK;
}

rt_status refit_mesh_on_devices(rt_scene *s, int32_t mesh, bool normals_changed, rt_mesh_quality *quality)
{
    rt::MeshData &m = s->data.meshes[mesh];
    bool any = false, measured = false;
    if (quality) { quality->flags = RT_MESH_QUALITY_NOT_ON_DEVICE; quality->cost = quality->built_cost = 0.0; quality->ratio = 1.0; quality->measure_ms = 0.0f; }
    for (DeviceState *D : s->devs) any = any || D->scene_valid;
    if (!any) return RT_OK;
    std::vector<DevObject> objs;
    std::vector<DevObjectBack> backs;
    std::vector<int32_t> node_mat;
    rt_status st = lower_objects(s->data, objs, backs, node_mat);
    int cur = 0;
    (void)hipGetDevice(&cur);
    rt_status ret = RT_OK;
    for (DeviceState *D : s->devs) {
        if (!D->scene_valid) continue;
        // a device another call is using, or one the update fails on, lowers the scene again at its next use instead
        DeviceClaim claim(D);
        rt_status r = st;
        if (!r && claim.ok) {
            // every device holds the same tree (the same host build, the same exact refit): the first one that refits measures it
            r = refit_mesh_on_device(D, m, mesh, normals_changed, objs, quality && !measured ? quality : nullptr);
            measured = measured || !r;
        }
        if (r || !claim.ok) D->scene_valid = false;
        if (r && !ret) ret = r;
    }
    (void)hipSetDevice(cur);
    // no device got as far as a measurement (all in use, or failed: they lower the scene again at their next use)
    if (quality && !measured) { quality->flags = RT_MESH_QUALITY_NOT_ON_DEVICE; quality->cost = quality->built_cost = 0.0; quality->ratio = 1.0; quality->measure_ms = 0.0f; }
    return ret;
}

// ---- mesh tree quality (rt_mi355x.h, "mesh tree quality") ------------------------------------------------------------------
// the host mirror: bvh_cost_host of rt_bvh_cost.h, the functions k_bvh_cost is made of, behind the ABI's argument checks
extern "C" rt_status rt_device_bvh_cost(const void *nodes, uint64_t n_nodes, uint32_t root_ref, double *cost, uint32_t *flags)
{
    if (!cost || !flags) return fail(RT_ERR_ARG, "rt_device_bvh_cost: NULL argument");
    if (!(root_ref & RT_COST_LEAF)) {
        if (root_ref >= n_nodes) return fail(RT_ERR_ARG, "rt_device_bvh_cost: root_ref names node %u of %llu", root_ref, (unsigned long long)n_nodes);
        if (!nodes) return fail(RT_ERR_ARG, "rt_device_bvh_cost: nodes is NULL");
        if (n_nodes > (1ull << 28)) return fail(RT_ERR_ARG, "rt_device_bvh_cost: %llu node records (a mesh has at most 2^28)", (unsigned long long)n_nodes);
    }
    bvh_cost_host(nodes, n_nodes, root_ref, cost, flags);
    return RT_OK;
}

// The measurement of mb's tree as it sits on D, queued on D's stream (the caller has claimed D and synchronises the stream before
// finish_mesh_cost): k_bvh_cost, then the block sums and the root's record to the host.  A mesh that is one leaf has nothing to launch.
static rt_status enqueue_mesh_cost(DeviceState *D, DevMeshBufs &mb)
{
    hipStream_t st = D->stream;
    for (Event &e : D->cost_ev) if (!e.e) HIP_TRY(e.create());
    HIP_TRY(hipEventRecord(D->cost_ev[0], st));
    if (!(mb.root_ref & RT_COST_LEAF)) {
        const uint64_t n_nodes = mb.level_off.back(), n_blocks = bvh_cost_blocks(n_nodes);
        rt_status rs;
        if ((rs = mb.cost_partials.ensure((n_blocks + 1) * sizeof(double)))) return rs;
        mb.cost_host.resize(n_blocks + 1 + sizeof(DevBvhNode) / sizeof(double));
        BvhCostRequest R = {};
        R.nodes = (const DevBvhNode *)mb.nodes.p; R.n_nodes = (uint32_t)n_nodes; R.partials = (double *)mb.cost_partials.p;
        HIP_TRY(rtk_launch_bvh_cost(st, R));
#if RT_COST_FOLD_DEVICE
        HIP_TRY(hipMemcpyAsync(mb.cost_host.data() + n_blocks, (const double *)mb.cost_partials.p + n_blocks, sizeof(double), hipMemcpyDeviceToHost, st));
#else
        HIP_TRY(hipMemcpyAsync(mb.cost_host.data(), mb.cost_partials.p, n_blocks * sizeof(double), hipMemcpyDeviceToHost, st));
#endif
        HIP_TRY(hipMemcpyAsync(mb.cost_host.data() + n_blocks + 1, (const DevBvhNode *)mb.nodes.p + mb.root_ref, sizeof(DevBvhNode), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipEventRecord(D->cost_ev[1], st));
    return RT_OK;
}
// ... and, the stream synchronised, what it says: the fold of the block sums in index order, the root box, the cost and its ratio
static rt_status finish_mesh_cost(DeviceState *D, const DevMeshBufs &mb, rt_mesh_quality *q)
{
    uint32_t flags = 0;
    if (mb.root_ref & RT_COST_LEAF) bvh_cost_host(nullptr, 0, mb.root_ref, &q->cost, &flags);
    else {
        const uint64_t n_blocks = bvh_cost_blocks(mb.level_off.back());
#if RT_COST_FOLD_DEVICE
        const double S = mb.cost_host[n_blocks];
#else
        const double S = bvh_cost_fold(mb.cost_host.data(), n_blocks);
#endif
        bvh_cost_finish(S, bvh_cost_root_half_area((const float *)(mb.cost_host.data() + n_blocks + 1)), &q->cost, &flags);
    }
    q->built_cost = mb.built_cost;
    if (flags || mb.built_flags) { q->flags = RT_MESH_QUALITY_DEGENERATE; q->cost = 0.0; q->ratio = 1.0; }
    else { q->flags = 0; q->ratio = q->cost / q->built_cost; }
    HIP_TRY(hipEventElapsedTime(&q->measure_ms, D->cost_ev[0], D->cost_ev[1]));
    return RT_OK;
}

// ---- device tree build (rt_mi355x.h, "device tree build") ---------------------------------------------------------------------
// the limit on a device-built tree's stack_need: what the kernels provide, or less under the test hook RT_LBVH_STACK_CAP (read at call time)
static int lbvh_stack_cap()
{
    int cap = RT_BVH_LDS + RT_BVH_SPILL;
    if (const char *e = getenv("RT_LBVH_STACK_CAP")) { const long v = strtol(e, nullptr, 10); if (v >= 0 && v < cap) cap = (int)v; }
    return cap;
}

// One device's share of rt_scene_update_mesh_vertices_build, modelled on refit_mesh_on_device: the same waits, the same uploads,
// then the tree built from the vertices just uploaded (rt_bvh_build.hip) in place of the refit, the slots written in its order, and
// everything that follows a tree's topology set again -- the record count and DevMesh::nodes / root_ref, slot_face, level_off and
// level_nodes, stack_need with DevScene::max_bvh_depth and the spill buffers, built_cost.  Two host synchronisations: one for
// the record count, the levels and stack_need (the cost launch and the fallback decision need them), one at the end.
// *fell_back: the tree needs more stack than `cap`; the device is left for the caller to invalidate.
static rt_status build_mesh_on_device(DeviceState *D, rt::MeshData &m, int32_t mesh, bool normals_changed, const std::vector<DevObject> &objs,
                                      int cap, rt_mesh_build_info *info, bool *fell_back)
{
    HIP_TRY(hipSetDevice(D->device));
    if (D->last_pending && D->last_done) HIP_TRY(hipEventSynchronize(D->last_done));      // an asynchronous render may still be tracing this mesh
    rt_status rs;
    if ((rs = motion_wait_host(D->device))) return rs;                                      // ... or k_motion_mesh walking it
    const size_t nf = m.f.size() / 3;
    if ((size_t)mesh >= D->mesh_bufs.size() || D->mesh_bufs[mesh].slot_face.size() != nf || objs.size() != (size_t)D->scene.n_objects)
        return fail(RT_ERR_STATE, "rt_scene_update_mesh_vertices_build: device %d does not hold mesh %d as the scene has it", D->device, mesh);
    DevMeshBufs &mb = D->mesh_bufs[mesh];
    MeshBuildBufs &B = D->build;
    hipStream_t st = D->stream;
    for (Event &e : B.ev) if (!e.e) HIP_TRY(e.create());
    const bool first = mb.vn.p == nullptr, first_build = mb.fn.p == nullptr;      // (f alone may be there already: k_mesh_normals reads it too)
    const bool smooth = m.normals_mode == RT_MESH_NORMALS_SMOOTH && !normals_changed;      // as in refit_mesh_on_device
    const bool textured = mb.tex.p != nullptr && !m.vt.empty() && m.ft.size() == m.f.size();
    if ((rs = mb.v.ensure(m.v.size() * 4)) || (rs = mb.vn.ensure(m.vn.size() * 4))) return rs;
    if (smooth && (rs = prepare_mesh_normals(D, m, mb))) return rs;
    if (first || normals_changed) ensure_normals(m);
    if (m.v_prev.empty()) mb.v_prev.release();
    else if ((rs = mb.v_prev.ensure(m.v_prev.size() * 4))) return rs;
    if (first_build) {
        if ((rs = mb.f.ensure(m.f.size() * 4)) || (rs = mb.fn.ensure(m.fn.size() * 4))) return rs;
        if (textured && ((rs = mb.ft.ensure(m.ft.size() * 4)) || (rs = mb.vt.ensure(m.vt.size() * 4)))) return rs;
    }
    // the scratch, and room for the records: fewer than nf (a record stands for a binary node with more than four keys beneath it)
    const uint32_t blocks = (uint32_t)((nf + 255) / 256);
    const size_t sort_bytes = rtk_mesh_build_sort_bytes((uint32_t)nf);
    if ((rs = B.cbox.ensure(((size_t)blocks + 1) * 24)) || (rs = B.keys[0].ensure(nf * 8)) || (rs = B.keys[1].ensure(nf * 8)) || (rs = B.sort_tmp.ensure(sort_bytes)) ||
        (rs = B.bin.ensure(nf * sizeof(LbvhBin))) || (rs = B.parent.ensure(nf * 4)) || (rs = B.visit.ensure(nf * 4)) || (rs = B.rec_bin.ensure(nf * 4)) ||
        (rs = B.rec_held.ensure(nf * 4)) || (rs = B.result.ensure(RT_LBVH_RESULT_WORDS * 4)) || (rs = B.slot_face.ensure(nf * 4))) return rs;
    if (nf > RT_LBVH_LEAF_TRIS && (rs = mb.nodes.ensure(nf * sizeof(DevBvhNode)))) return rs;      // (may move: DevMesh::nodes is set again below)
    if ((rs = mb.level_nodes.ensure(nf * 4))) return rs;
    HIP_TRY(hipEventRecord(B.ev[0], st));
    if (!m.v_prev.empty()) HIP_TRY(hipMemcpyAsync(mb.v_prev.p, m.v_prev.data(), m.v_prev.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(mb.v.p, m.v.data(), m.v.size() * 4, hipMemcpyHostToDevice, st));
    if (first || normals_changed) HIP_TRY(hipMemcpyAsync(mb.vn.p, m.vn.data(), m.vn.size() * 4, hipMemcpyHostToDevice, st));
    if (first_build) {
        HIP_TRY(hipMemcpyAsync(mb.f.p, m.f.data(), m.f.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(mb.fn.p, m.fn.data(), m.fn.size() * 4, hipMemcpyHostToDevice, st));
        if (textured) {
            HIP_TRY(hipMemcpyAsync(mb.ft.p, m.ft.data(), m.ft.size() * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(mb.vt.p, m.vt.data(), m.vt.size() * 4, hipMemcpyHostToDevice, st));
        }
    }
    if (smooth && (rs = enqueue_mesh_normals(D, m, mb))) return rs;      // k_mesh_retri, behind the build, copies them into the slots
    HIP_TRY(hipEventRecord(B.ev[1], st));
    MeshBuildRequest R = {};
    R.v = (const float *)mb.v.p; R.f = (const uint32_t *)mb.f.p; R.fn = (const uint32_t *)mb.fn.p; R.n_faces = (uint32_t)nf;
    if (textured) { R.vt = (const float *)mb.vt.p; R.ft = (const uint32_t *)mb.ft.p; R.tex = (float *)mb.tex.p; }
    R.scratch.cbox = (float *)B.cbox.p; R.scratch.keys[0] = (unsigned long long *)B.keys[0].p; R.scratch.keys[1] = (unsigned long long *)B.keys[1].p;
    R.scratch.sort_tmp = B.sort_tmp.p; R.scratch.sort_tmp_bytes = sort_bytes;
    R.scratch.bin = (LbvhBin *)B.bin.p; R.scratch.parent = (uint32_t *)B.parent.p; R.scratch.visit = (uint32_t *)B.visit.p;
    R.scratch.rec_bin = (uint32_t *)B.rec_bin.p; R.scratch.rec_held = (int32_t *)B.rec_held.p;
    R.nodes = (DevBvhNode *)mb.nodes.p; R.result = (uint32_t *)B.result.p;
    R.slot_face = (uint32_t *)B.slot_face.p; R.slot_idx = (uint32_t *)mb.slot_idx.p;
    R.after_sort = B.ev[2]; R.after_boxes = B.ev[3]; R.after_collapse = B.ev[4];
    int launches = 0;
    HIP_TRY(rtk_launch_mesh_build(st, R, &launches));
    MeshRefitRequest T = {};                                     // k_mesh_retri alone: no level of the old tree is refitted
    T.v = R.v; T.vn = (const float *)mb.vn.p; T.slot_idx = R.slot_idx; T.n_slots = (uint32_t)nf;
    T.tris = (DevTri *)mb.tris.p; T.nrm = (float *)mb.nrm.p;
    HIP_TRY(rtk_launch_mesh_refit(st, T));
    launches++;
    HIP_TRY(hipEventRecord(B.ev[5], st));
    B.result_host.assign(RT_LBVH_RESULT_WORDS, 0u);
    B.slot_face_host.resize(nf);
    HIP_TRY(hipMemcpyAsync(B.result_host.data(), B.result.p, RT_LBVH_RESULT_WORDS * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(B.slot_face_host.data(), B.slot_face.p, nf * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint32_t n_nodes = B.result_host[0], levels = B.result_host[1];
    const int need = (int)B.result_host[2];
    if (info) {
        info->n_nodes = n_nodes; info->n_slots = (uint32_t)nf; info->stack_need = need; info->levels = (int32_t)levels;
        info->root_ref = nf <= RT_LBVH_LEAF_TRIS ? lbvh_leafref(0, (uint32_t)nf) : 0u;
        info->launches = launches; info->syncs = 1;
        HIP_TRY(hipEventElapsedTime(&info->upload_ms, B.ev[0], B.ev[1]));
        HIP_TRY(hipEventElapsedTime(&info->sort_ms, B.ev[1], B.ev[2]));
        HIP_TRY(hipEventElapsedTime(&info->hierarchy_ms, B.ev[2], B.ev[3]));
        HIP_TRY(hipEventElapsedTime(&info->collapse_ms, B.ev[3], B.ev[4]));
        HIP_TRY(hipEventElapsedTime(&info->slots_ms, B.ev[4], B.ev[5]));
    }
    if (B.result_host[3] || need > cap || n_nodes > nf || levels > RT_LBVH_MAX_LEVELS) { *fell_back = true; return RT_OK; }
    // what follows the topology, on the host: slot order, root, need, the levels as the refit wants them (deepest first; numbering
    // is breadth-first, so depth d is the index range [at[d], at[d + 1]) and level_nodes is those ranges in reverse order)
    const uint32_t *at = B.result_host.data() + 4;
    mb.slot_face = B.slot_face_host;
    mb.root_ref = nf <= RT_LBVH_LEAF_TRIS ? lbvh_leafref(0, (uint32_t)nf) : 0u;
    mb.stack_need = need;
    mb.level_off.assign((size_t)levels + 1, 0u);
    B.level_nodes_host.resize(n_nodes);
    for (uint32_t k = 0, w = 0; k < levels; k++) {
        const uint32_t d = levels - 1 - k;
        for (uint32_t i = at[d]; i < at[d + 1]; i++) B.level_nodes_host[w++] = i;
        mb.level_off[k + 1] = mb.level_off[k] + (at[d + 1] - at[d]);
    }
    if (n_nodes) HIP_TRY(hipMemcpyAsync(mb.level_nodes.p, B.level_nodes_host.data(), (size_t)n_nodes * 4, hipMemcpyHostToDevice, st));
    DevMesh dm;
    memset(&dm, 0, sizeof dm);
    dm.nodes = (const DevBvhNode *)mb.nodes.p; dm.tris = (const DevTri *)mb.tris.p; dm.nrm = (const float *)mb.nrm.p;
    dm.tex = textured ? (const float *)mb.tex.p : nullptr;
    dm.root_ref = mb.root_ref; dm.n_tris = (uint32_t)nf;
    memcpy(dm.root_box, m.root_box, 24);
    HIP_TRY(hipMemcpyAsync((char *)D->meshes.p + (size_t)mesh * sizeof(DevMesh), &dm, sizeof(DevMesh), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(D->objects.p, objs.data(), objs.size() * sizeof(DevObject), hipMemcpyHostToDevice, st));
    if (need > D->scene.max_bvh_depth) {                        // the spill buffers come into being as in upload_scene and ensure_workspace
        D->scene.max_bvh_depth = need;
        if (need > RT_BVH_LDS) {
            if ((rs = D->bvh_spill.ensure(SPILL_BYTES))) return rs;
            D->scene.bvh_spill = (uint32_t *)D->bvh_spill.p;
            for (Workspace &w : D->ws) if (w.samples && (rs = w.bvh_spill.ensure(SPILL_BYTES))) return rs;
        }
    }
    D->upd_levels = -1;                                         // (rt_scene_mesh_update_ms speaks of refits)
    if ((rs = enqueue_mesh_cost(D, mb))) return rs;
    HIP_TRY(hipStreamSynchronize(st));
    rt_mesh_quality q = {};
    mb.built_cost = 1.0; mb.built_flags = 0;
    if ((rs = finish_mesh_cost(D, mb, &q))) return rs;
    mb.built_cost = q.cost; mb.built_flags = (q.flags & RT_MESH_QUALITY_DEGENERATE) ? RT_COST_DEGENERATE : 0u;
    if (info) { info->cost = q.cost; info->cost_ms = q.measure_ms; info->launches = launches + (n_nodes ? 1 : 0); info->syncs = 2; }
    return RT_OK;
}

rt_status build_mesh_on_devices(rt_scene *s, int32_t mesh, bool normals_changed, rt_mesh_build_info *info)
{
    rt::MeshData &m = s->data.meshes[mesh];
    rt_mesh_build_info none = {};
    none.struct_size = sizeof none; none.flags = RT_MESH_BUILD_NOT_ON_DEVICE;
    *info = none;
    bool any = false, reported = false, fell_back = false;
    for (DeviceState *D : s->devs) any = any || D->scene_valid;
    if (!any) return RT_OK;
    std::vector<DevObject> objs;
    std::vector<DevObjectBack> backs;
    std::vector<int32_t> node_mat;
    rt_status st = lower_objects(s->data, objs, backs, node_mat);
    const int cap = lbvh_stack_cap();
    int cur = 0;
    (void)hipGetDevice(&cur);
    rt_status ret = RT_OK;
    for (DeviceState *D : s->devs) {
        if (!D->scene_valid) continue;
        // a device another call is using, or one the build fails on, lowers the scene again at its next use instead
        DeviceClaim claim(D);
        rt_status r = st;
        if (!r && claim.ok && !fell_back) {
            rt_mesh_build_info mine = none;
            r = build_mesh_on_device(D, m, mesh, normals_changed, objs, cap, &mine, &fell_back);
            if (!r && !reported) { *info = mine; info->flags = fell_back ? RT_MESH_BUILD_FELL_BACK : RT_MESH_BUILD_ON_DEVICE; reported = true; }
        }
        if (r || !claim.ok || fell_back) D->scene_valid = false;
        if (r && !ret) ret = r;
    }
    (void)hipSetDevice(cur);
    // the same mesh gives the same tree on every device: one that does not fit fits nowhere, and the call takes REBUILD's path
    if (fell_back) { s->invalidate(true, false); info->flags = RT_MESH_BUILD_FELL_BACK; }
    return ret;
}

extern "C" rt_status rt_scene_mesh_quality(rt_scene *s, int device, int32_t mesh, rt_mesh_quality *out)
{
    if (!s || !out) return fail(RT_ERR_ARG, "rt_scene_mesh_quality: NULL argument");
    if (out->struct_size != sizeof(rt_mesh_quality))
        return fail(RT_ERR_ARG, "rt_scene_mesh_quality: rt_mesh_quality.struct_size is %u, this library's is %zu", out->struct_size, sizeof(rt_mesh_quality));
    {
        std::lock_guard<std::mutex> lk(s->mu);
        if (mesh < 0 || (size_t)mesh >= s->data.meshes.size() || s->data.meshes[mesh].f.empty()) return fail(RT_ERR_ARG, "rt_scene_mesh_quality: mesh %d was never set", mesh);
    }
    DeviceState *D = nullptr;
    rt_status st = prepare_device(s, device, &D);
    if (st) return st;
    DeviceClaim claim(D);
    if (!claim.ok) return fail(RT_ERR_STATE, "rt_scene_mesh_quality: another call on this scene is using device %d", device);
    if (D->last_pending && D->last_done) HIP_TRY(hipEventSynchronize(D->last_done));
    DevMeshBufs &mb = D->mesh_bufs[mesh];
    if ((st = enqueue_mesh_cost(D, mb))) return st;
    HIP_TRY(hipStreamSynchronize(D->stream));
    return finish_mesh_cost(D, mb, out);
}

extern "C" rt_status rt_scene_mesh_update_ms(rt_scene *s, int device, rt_mesh_update_ms *out)
{
    if (!s || !out) return fail(RT_ERR_ARG, "rt_scene_mesh_update_ms: NULL argument");
    if (out->struct_size != sizeof(rt_mesh_update_ms))
        return fail(RT_ERR_ARG, "rt_scene_mesh_update_ms: rt_mesh_update_ms.struct_size is %u, this library's is %zu", out->struct_size, sizeof(rt_mesh_update_ms));
    DeviceState *D = find_device_state(s, device);
    if (!D || D->upd_levels < 0) return fail(RT_ERR_STATE, "rt_scene_mesh_update_ms: device %d has not updated a mesh in place", device);
    HIP_TRY(hipEventElapsedTime(&out->upload, D->upd_ev[0], D->upd_ev[1]));
    HIP_TRY(hipEventElapsedTime(&out->retri, D->upd_ev[1], D->upd_ev[2]));
    HIP_TRY(hipEventElapsedTime(&out->refit, D->upd_ev[2], D->upd_ev[3]));
    out->level_launches = D->upd_levels;
    return RT_OK;
}

extern "C" rt_status rt_scene_mesh_normals_ms(rt_scene *s, int device, float *ms)
{
    if (!s || !ms) return fail(RT_ERR_ARG, "rt_scene_mesh_normals_ms: NULL argument");
    DeviceState *D = find_device_state(s, device);
    if (!D || !D->nrm_timed) return fail(RT_ERR_STATE, "rt_scene_mesh_normals_ms: device %d has not computed a mesh's normals", device);
    HIP_TRY(hipEventElapsedTime(ms, D->nrm_ev[0], D->nrm_ev[1]));
    return RT_OK;
}

extern "C" rt_status rt_scene_mesh_device_read(rt_scene *s, int device, int32_t mesh, rt_device_bvh_info *info, void *nodes, uint64_t nodes_cap,
                                               uint32_t *slot_face, uint64_t slots_cap, float *tris, float *nrm, float root_box[6])
{
    if (!s || !info) return fail(RT_ERR_ARG, "rt_scene_mesh_device_read: NULL argument");
    if (info->struct_size != sizeof(rt_device_bvh_info))
        return fail(RT_ERR_ARG, "rt_scene_mesh_device_read: rt_device_bvh_info.struct_size is %u, this library's is %zu", info->struct_size, sizeof(rt_device_bvh_info));
    {
        std::lock_guard<std::mutex> lk(s->mu);
        if (mesh < 0 || (size_t)mesh >= s->data.meshes.size() || s->data.meshes[mesh].f.empty()) return fail(RT_ERR_ARG, "rt_scene_mesh_device_read: mesh %d was never set", mesh);
    }
    DeviceState *D = nullptr;
    rt_status st = prepare_device(s, device, &D);
    if (st) return st;
    DeviceClaim claim(D);
    if (!claim.ok) return fail(RT_ERR_STATE, "rt_scene_mesh_device_read: another call on this scene is using device %d", device);
    if (D->last_pending && D->last_done) HIP_TRY(hipEventSynchronize(D->last_done));
    const DevMeshBufs &mb = D->mesh_bufs[mesh];
    const size_t n_slots = mb.slot_face.size(), n_nodes = mb.level_off.empty() ? 0 : mb.level_off.back();
    if (nodes && nodes_cap < n_nodes) return fail(RT_ERR_ARG, "rt_scene_mesh_device_read: room for %llu node records, %zu needed", (unsigned long long)nodes_cap, n_nodes);
    if ((slot_face || tris || nrm) && slots_cap < n_slots) return fail(RT_ERR_ARG, "rt_scene_mesh_device_read: room for %llu triangle slots, %zu needed", (unsigned long long)slots_cap, n_slots);
    HIP_TRY(hipStreamSynchronize(D->stream));
    if (nodes && n_nodes) HIP_TRY(hipMemcpy(nodes, mb.nodes.p, n_nodes * sizeof(DevBvhNode), hipMemcpyDeviceToHost));
    if (tris) HIP_TRY(hipMemcpy(tris, mb.tris.p, n_slots * sizeof(DevTri), hipMemcpyDeviceToHost));
    if (nrm) HIP_TRY(hipMemcpy(nrm, mb.nrm.p, n_slots * 36, hipMemcpyDeviceToHost));
    if (root_box) HIP_TRY(hipMemcpy(root_box, (const char *)D->meshes.p + (size_t)mesh * sizeof(DevMesh) + offsetof(DevMesh, root_box), 24, hipMemcpyDeviceToHost));
    if (slot_face) memcpy(slot_face, mb.slot_face.data(), n_slots * 4);
    info->n_nodes = (uint32_t)n_nodes; info->n_slots = (uint32_t)n_slots;
    info->root_ref = mb.root_ref; info->stack_need = mb.stack_need;
    info->bvh_lds = RT_BVH_LDS; info->bvh_stack = RT_BVH_STACK; info->bvh_spill = RT_BVH_SPILL;
    info->spill_blocks = RT_SPILL_BLOCKS; info->block = RT_BLOCK;
    return RT_OK;
}

// the previous positions of one mesh as they sit on `device`, with rt_scene_mesh_device_read's discipline
extern "C" rt_status rt_scene_mesh_device_previous(rt_scene *s, int device, int32_t mesh, float *v_prev, uint64_t nv_cap, uint32_t *nv_out)
{
    if (!s || !nv_out) return fail(RT_ERR_ARG, "rt_scene_mesh_device_previous: NULL argument");
    size_t nv = 0;
    {
        std::lock_guard<std::mutex> lk(s->mu);
        if (mesh < 0 || (size_t)mesh >= s->data.meshes.size() || s->data.meshes[mesh].f.empty()) return fail(RT_ERR_ARG, "rt_scene_mesh_device_previous: mesh %d was never set", mesh);
        nv = s->data.meshes[mesh].v.size() / 3;
    }
    DeviceState *D = nullptr;
    rt_status st = prepare_device(s, device, &D);
    if (st) return st;
    DeviceClaim claim(D);
    if (!claim.ok) return fail(RT_ERR_STATE, "rt_scene_mesh_device_previous: another call on this scene is using device %d", device);
    if (D->last_pending && D->last_done) HIP_TRY(hipEventSynchronize(D->last_done));
    const DevMeshBufs &mb = D->mesh_bufs[mesh];
    if (!mb.v_prev.p) { *nv_out = 0; return RT_OK; }
    if (v_prev && nv_cap < nv) return fail(RT_ERR_ARG, "rt_scene_mesh_device_previous: room for %llu vertices, %zu needed", (unsigned long long)nv_cap, nv);
    HIP_TRY(hipStreamSynchronize(D->stream));
    if (v_prev) HIP_TRY(hipMemcpy(v_prev, mb.v_prev.p, nv * 12, hipMemcpyDeviceToHost));
    *nv_out = (uint32_t)nv;
    return RT_OK;
}

rt_status prepare_device(rt_scene *s, int device, DeviceState **out)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return fail(RT_ERR_NO_DEVICE, "no HIP device is visible (this library has no CPU path)"); }
    if (device < 0 || device >= n) return fail(RT_ERR_ARG, "device %d out of range (0..%d)", device, n - 1);
    if (!device_is_gfx950(device)) return fail(RT_ERR_NO_DEVICE, "device %d is not gfx950 (MI355X); kernels are built for gfx950 only", device);
    HIP_TRY(hipSetDevice(device));
    std::lock_guard<std::mutex> lk(s->mu);
    DeviceState *D = device_state(s, device);
    if (!D->stream) HIP_TRY(hipStreamCreateWithFlags(&D->stream, hipStreamNonBlocking));
    rt_status st;
    // an asynchronous render (sync == 0) may still be reading the buffers an upload is about to overwrite (scene tables and
    // photon structure are re-used in place when the new data fits): wait for it on the host first
    if ((!D->scene_valid || !D->maps[0].valid || !D->maps[1].valid) && D->last_pending && D->last_done) HIP_TRY(hipEventSynchronize(D->last_done));
    if (!D->scene_valid && (st = motion_wait_host(device))) return st;      // (k_motion_mesh reads the scene tables and the meshes, not the photon maps)
    if (!D->scene_valid) { const DevPhotonMap keep = D->scene.pm, keepc = D->scene.cm; if ((st = upload_scene(s, D))) return st; D->scene.pm = keep; D->scene.cm = keepc; }
    for (int caustic = 0; caustic < 2; caustic++)
        if (!D->maps[caustic].valid && (st = upload_photons(s, D, caustic != 0))) return st;
    *out = D;
    return RT_OK;
}
