// rt_lower.cpp -- what puts a scene on a device: the lowering of the scene store (rt_api.cpp) to the device layout of rt_dev.h and
// the tree the kernels walk.  prepare_device has rt_photons.cpp put the two photon maps beside it; rt_render.cpp renders from
// what it leaves, rt_mesh_update.cpp changes a mesh of it in place; rt_host.h is what the host files share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/rt_mi355x.h"
#include "host/rt_scene.h"
#include "rt_host.h"
#include "rt_bvh_cost.h"

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
        rt_status st = check_mesh_set(s, mesh, "rt_scene_mesh_device_bvh");
        if (st) return st;
        st = build_sah_bvh(s->data.meshes[mesh], bn, faces, root_ref, need);
        if (st) return st;
    }
    // both capacities before anything is written: a refused call leaves info and both buffers as they were
    if (nodes && nodes_cap < bn.size()) return fail(RT_ERR_ARG, "rt_scene_mesh_device_bvh: room for %llu node records, %zu needed", (unsigned long long)nodes_cap, bn.size());
    if (slot_face && slots_cap < faces.size()) return fail(RT_ERR_ARG, "rt_scene_mesh_device_bvh: room for %llu triangle slots, %zu needed", (unsigned long long)slots_cap, faces.size());
    fill_device_bvh_info(info, bn.size(), faces.size(), root_ref, need);
    if (nodes) memcpy(nodes, bn.data(), bn.size() * sizeof(DevBvhNode));
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
// in-place mesh update (rt_mesh_update.cpp), which moves the cull boxes of the objects whose mesh changed.
rt_status lower_objects(const rt::SceneData &sd, std::vector<DevObject> &objs, std::vector<DevObjectBack> &backs, std::vector<int32_t> &node_mat)
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
    // a posed mesh (rt_mi355x.h, "mesh skinning"): its positions and root box, which everything below reads, are the pose's
    for (rt::MeshData &m : s->data.meshes) ensure_vertices(m);
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
