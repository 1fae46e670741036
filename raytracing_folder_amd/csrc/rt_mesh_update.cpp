// rt_mesh_update.cpp -- everything that changes a lowered mesh in place: the six rt_scene_update_mesh_vertices*, the four
// rt_scene_pose_mesh* and the four rt_scene_morph_mesh* entry points on one entry path, their share of the scene store, and what
// they do on the devices that hold the scene -- the refit (rt_refit.hip), the refitted tree's quality (k_bvh_cost), the device tree
// build (rt_bvh_build.hip), smooth normals (rt_mesh_normals.hip), a pose by bones, morph targets or both (rt_mesh_pose.hip) -- behind
// one per-device upload and one loop over the devices; the host mirrors of the cost and of the build; the calls that read a mesh
// back from a device.  rt_lower.cpp put the mesh there (upload_scene); rt_host.h is what the host files share.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <optional>
#include <vector>

#include "../../include/rt_mi355x.h"
#include "host/rt_scene.h"
#include "rt_host.h"
#include "rt_bvh_cost.h"
#include "rt_lbvh.h"
#include "rt_mesh_normals.h"

// ---- the store's share -----------------------------------------------------------------------------------------------------
// Where an entry point's new vertices come from: the array it brought (with normals, or without), a bone pose of the mesh's skin
// (rt_scene_pose_mesh*), or a morph pose of its morph set (rt_scene_morph_mesh*): weights, and bones that may be NULL
enum InputKind { INPUT_VERTICES, INPUT_BONE_POSE, INPUT_MORPH_POSE };
struct MeshInput {
    InputKind kind;
    const float *v; int32_t nv; const float *vn; int32_t nvn;
    const float *bones; int32_t n_bones; const float *weights; int32_t n_targets;
};
static MeshInput input_vertices(const float *v, int32_t nv, const float *vn, int32_t nvn) { return {INPUT_VERTICES, v, nv, vn, nvn, nullptr, 0, nullptr, 0}; }
static MeshInput input_bones(const float *bones, int32_t n_bones) { return {INPUT_BONE_POSE, nullptr, 0, nullptr, 0, bones, n_bones, nullptr, 0}; }
static MeshInput input_morphs(const float *weights, int32_t n_targets, const float *bones, int32_t n_bones)
{
    return {INPUT_MORPH_POSE, nullptr, 0, nullptr, 0, bones, n_bones, weights, n_targets};
}

// What the entry points share once their arguments have passed: the checks against the mesh (`who` names the entry point in
// the message) and the new vertices in the store.  keep_previous (RT_MESH_UPDATE_KEEP_PREVIOUS): the positions the mesh had
// become its previous positions; without it the mesh holds none afterwards.  The caller holds s->mu.
static rt_status store_mesh_vertices(rt_scene *s, int32_t mesh, const MeshInput &in, bool keep_previous, const char *who)
{
    rt_status st = check_mesh_set(s, mesh, who);
    if (st) return st;
    rt::MeshData &m = s->data.meshes[mesh];
    if ((size_t)in.nv != m.v.size() / 3 || in.nv < 0) return fail(RT_ERR_ARG, "%s: nv is %d, the mesh has %zu vertices (the faces stay as they are)", who, in.nv, m.v.size() / 3);
    if ((in.vn || in.nvn != 0) && ((size_t)in.nvn != m.vn.size() / 3 || in.nvn < 0))
        return fail(RT_ERR_ARG, "%s: nvn is %d, the mesh has %zu normals", who, in.nvn, m.vn.size() / 3);
    // (a posed mesh: positions a pose still owes are resolved before they become the previous ones, and dropped otherwise)
    if (keep_previous) { ensure_vertices(m); m.v_prev.swap(m.v); } else { std::vector<float>().swap(m.v_prev); m.v_prev_stale = false; }
    m.v.assign(in.v, in.v + 3 * (size_t)in.nv);
    m.v_stale = false;
    // SMOOTH mode without normals: the devices compute them (begin_mesh_update), the store when they are next read -- not here
    if (in.vn) { m.vn.assign(in.vn, in.vn + 3 * (size_t)in.nvn); m.vn_stale = false; }
    else if (m.normals_mode == RT_MESH_NORMALS_SMOOTH) m.vn_stale = true;
    m.tree_stale = true;
    rt::MeshRootBox(m.v.data(), m.f.data(), (unsigned)(m.f.size() / 3), m.root_box);
    // a generated photon map was traced through the old shape (geometry_changed); the scene itself stays where it is refitted
    s->drop_generated_photons();
    return RT_OK;
}

// ... and a pose in the store (rt_mi355x.h, "mesh skinning", "morph targets"): each kind's checks, then the pose -- bones, or
// weights and the bones if any came -- and a mark, no per-vertex work: v is owed from then on (ensure_vertices), and so is root_box
// unless a device reports it.
static rt_status store_mesh_pose(rt_scene *s, int32_t mesh, const MeshInput &in, bool keep_previous, const char *who)
{
    rt_status st = check_mesh_set(s, mesh, who);
    if (st) return st;
    rt::MeshData &m = s->data.meshes[mesh];
    const bool morph = in.kind == INPUT_MORPH_POSE, skinned = !morph || in.bones;
    if (!morph) {
        if (m.skin_bones == 0) return fail(RT_ERR_STATE, "%s: mesh %d has no skin (rt_scene_set_mesh_skin binds one)", who, mesh);
        if (in.n_bones != m.skin_bones) return fail(RT_ERR_ARG, "%s: n_bones is %d, the skin has %d", who, in.n_bones, m.skin_bones);
        if ((st = check_pose(who, in.bones, in.n_bones))) return st;
    } else {
        if (m.morph_targets == 0) return fail(RT_ERR_STATE, "%s: mesh %d has no morph set (rt_scene_set_mesh_morphs binds one)", who, mesh);
        if (in.bones && m.skin_bones == 0) return fail(RT_ERR_STATE, "%s: bones given and mesh %d has no skin (rt_scene_set_mesh_skin binds one)", who, mesh);
        if (in.n_targets != m.morph_targets) return fail(RT_ERR_ARG, "%s: n_targets is %d, the morph set has %d", who, in.n_targets, m.morph_targets);
        if (!in.bones && in.n_bones != 0) return fail(RT_ERR_ARG, "%s: bones is NULL and n_bones is %d", who, in.n_bones);
        if (in.bones && in.n_bones != m.skin_bones) return fail(RT_ERR_ARG, "%s: n_bones is %d, the skin has %d", who, in.n_bones, m.skin_bones);
        if ((st = check_finite(who, "weights", in.weights, in.n_targets)) || (in.bones && (st = check_pose(who, in.bones, in.n_bones)))) return st;
    }
    // keep_previous, three cases: none kept; v is owed itself, and the pose it is owed from is handed on, not the vertices; the
    // store has v, which becomes v_prev where it is
    if (!keep_previous) { std::vector<float>().swap(m.v_prev); m.v_prev_stale = false; }
    else if (m.v_stale) {
        m.pose_prev = m.pose;
        if (m.v_prev.size() != m.v.size()) m.v_prev.resize(m.v.size());
        m.v_prev_stale = true;
    } else {
        m.v_prev.swap(m.v);
        m.v_prev_stale = false;
        if (m.v.size() != m.v_prev.size()) m.v.resize(m.v_prev.size());
    }
    m.pose.morphed = morph; m.pose.skinned = skinned;
    if (morph) m.pose.weights.assign(in.weights, in.weights + in.n_targets);      // (the other kind's last array stays: it is not read)
    if (skinned) m.pose.bones.assign(in.bones, in.bones + 12 * (size_t)in.n_bones);
    m.v_stale = true;
    if (m.normals_mode == RT_MESH_NORMALS_SMOOTH) m.vn_stale = true;
    m.tree_stale = true;
    s->drop_generated_photons();
    return RT_OK;
}

// ---- one device's upload ---------------------------------------------------------------------------------------------------
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

// A pose (rt_mi355x.h, "mesh skinning", "morph targets"), one device's share in the same two steps, whatever the pose's kind.
// prepare: what the kind reads, on the device from the mesh's first pose of that kind there -- the skin (rest pose, indices,
// weights) and room for the bones if the pose has bones, the morph set (base, deltas) and room for the active list if it has
// weights.  enqueue: the active list (compacted here: 8 bytes a non-zero weight), the bones (48 bytes each), and ONE launch of
// k_mesh_pose on the update's stream, in place of the vertex upload and ahead of k_mesh_normals, between the events of the kind:
// a bone pose times into rt_scene_mesh_skin_ms, a morph pose -- with bones or without -- into rt_scene_mesh_morph_ms.
static rt_status prepare_mesh_pose(DeviceState *D, const rt::MeshData &m, DevMeshBufs &mb)
{
    const rt::MeshPose &p = m.pose;
    rt_status rs;
    for (Event &e : D->pose_ev[p.morphed]) if (!e.e) HIP_TRY(e.create());
    if (p.morphed && (rs = D->morph_active.ensure(sizeof(D->morph_active_host)))) return rs;
    if (p.skinned) {
        if ((rs = D->skin_bones.ensure(p.bones.size() * 4))) return rs;
        if (!mb.skin_rest.p || mb.skin_serial != m.skin_serial) {
            if ((rs = mb.skin_rest.upload(m.skin_rest.data(), m.skin_rest.size() * 4)) || (rs = mb.skin_index.upload(m.skin_index.data(), m.skin_index.size() * 2)) ||
                (rs = mb.skin_weight.upload(m.skin_weight.data(), m.skin_weight.size() * 4))) return rs;
            mb.skin_serial = m.skin_serial;
        }
    }
    if (p.morphed && (!mb.morph_base.p || mb.morph_serial != m.morph_serial)) {
        if ((rs = mb.morph_base.upload(m.morph_base.data(), m.morph_base.size() * 4)) || (rs = mb.morph_deltas.upload(m.morph_deltas.data(), m.morph_deltas.size() * 4))) return rs;
        mb.morph_serial = m.morph_serial;
    }
    return RT_OK;
}
static rt_status enqueue_mesh_pose(DeviceState *D, const rt::MeshData &m, DevMeshBufs &mb)
{
    const rt::MeshPose &p = m.pose;
    MeshPoseRequest K = {};
    K.base = (const float *)(p.morphed ? mb.morph_base.p : mb.skin_rest.p);
    K.nv = (uint32_t)(m.v.size() / 3); K.out = (float *)mb.v.p;
    if (p.morphed) {
        K.deltas = (const float *)mb.morph_deltas.p; K.active = D->morph_active.p;
        K.n_active = mesh_morph_compact(p.weights.data(), (uint32_t)m.morph_targets, D->morph_active_host);
        if (K.n_active) HIP_TRY(hipMemcpyAsync(D->morph_active.p, D->morph_active_host, K.n_active * sizeof(MeshMorphActive), hipMemcpyHostToDevice, D->stream));
    }
    if (p.skinned) {
        K.bone_index = (const uint16_t *)mb.skin_index.p; K.weight = (const float *)mb.skin_weight.p;
        K.bones = (const float *)D->skin_bones.p; K.n_bones = (uint32_t)m.skin_bones;
        HIP_TRY(hipMemcpyAsync(D->skin_bones.p, p.bones.data(), p.bones.size() * 4, hipMemcpyHostToDevice, D->stream));
    }
    HIP_TRY(hipEventRecord(D->pose_ev[p.morphed][0], D->stream));
    HIP_TRY(rtk_launch_mesh_pose(D->stream, K));
    HIP_TRY(hipEventRecord(D->pose_ev[p.morphed][1], D->stream));
    D->pose_timed[p.morphed] = true;
    return RT_OK;
}
void release_mesh_binding_on_devices(rt_scene *s, int32_t mesh, MeshBinding which)
{
    const bool morphs = which == BINDING_MORPHS;
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (DeviceState *D : s->devs) {
        if ((size_t)mesh >= D->mesh_bufs.size()) continue;
        DevMeshBufs &mb = D->mesh_bufs[mesh];
        if ((morphs ? mb.morph_base.p : mb.skin_rest.p) && hipSetDevice(D->device) == hipSuccess) { if (morphs) mb.release_morphs(); else mb.release_skin(); }
    }
    if (!s->devs.empty()) (void)hipSetDevice(cur);
}

// Where an update's new vertices come from on a device: the store (uploaded), the pose the store holds (k_mesh_pose writes them
// from its bones, its weights or both), or nowhere -- they are on the device already, behind the refit of the same call.  From a
// pose the host has no positions, so a flagged pose swaps pointers and the root box is read back.
enum VertexSource { VERTICES_FROM_STORE, VERTICES_FROM_POSE, VERTICES_ON_DEVICE };

// the box of a tree's root record: per axis the smallest lo and the largest hi over its used children (lo[axis][child],
// hi[axis][child]; an unused child has a NaN lo on x) -- the exact min / max of the vertices under the faces, MeshRootBox's box
static void root_box_of_record(const float *rec, float box[6])
{
    bool any = false;
    for (uint32_t c = 0; c < 4; c++) {
        if (rec[c] != rec[c]) continue;
        for (int a = 0; a < 3; a++) {
            const float l = rec[4 * a + c], h = rec[12 + 4 * a + c];
            if (!any || l < box[a]) box[a] = l;
            if (!any || h > box[a + 3]) box[a + 3] = h;
        }
        any = true;
    }
}
// the objects lowered again once a posed mesh's root box is known (the first device's tail; the later devices get these)
static rt_status relower_objects(const rt::SceneData &sd, std::vector<DevObject> &objs)
{
    std::vector<DevObjectBack> backs;
    std::vector<int32_t> node_mat;
    return lower_objects(sd, objs, backs, node_mat);
}

// tex of the mesh follows texture vertices the store still has (a device build writes it again from them)
static bool mesh_textured(const DevMeshBufs &mb, const rt::MeshData &m) { return mb.tex.p != nullptr && !m.vt.empty() && m.ft.size() == m.f.size(); }

// What a refit and a device build share on one device, up to the point where the new vertices (and normals) are on it: the two
// host waits, the check that the device holds the mesh as the scene has it (`who`: the entry family the message names), the
// buffers, the upload between ev[0] and ev[1] (ev: the caller's n_ev events, all made here), smooth normals behind it.
// with_faces: the device build's arrays -- f, fn and, for a textured mesh, ft and vt -- on the device from the mesh's first build
// there.  reserve (may be empty): what else the caller's tail allocates, ahead of ev[0] so that nothing is allocated between
// the events.  src: VERTICES_FROM_POSE puts the pose -- the active list, 48 bytes a bone -- and k_mesh_pose in the vertex upload's
// place, and a flagged pose makes the buffer the positions were in the previous positions' -- two pointers swapped, nothing
// uploaded; VERTICES_ON_DEVICE leaves positions and previous positions as the refit of the same call left them.
static rt_status begin_mesh_update(DeviceState *D, rt::MeshData &m, int32_t mesh, bool normals_changed, size_t n_objects, const char *who,
                                   Event *ev, size_t n_ev, bool with_faces, const std::function<rt_status()> &reserve,
                                   VertexSource src = VERTICES_FROM_STORE)
{
    HIP_TRY(hipSetDevice(D->device));
    if (D->last_pending && D->last_done) HIP_TRY(hipEventSynchronize(D->last_done));      // an asynchronous render may still be tracing this mesh
    rt_status rs;
    if ((rs = motion_wait_host(D->device))) return rs;                                      // ... or k_motion_mesh walking it
    if ((size_t)mesh >= D->mesh_bufs.size() || D->mesh_bufs[mesh].slot_face.size() != m.f.size() / 3 || n_objects != (size_t)D->scene.n_objects)
        return fail(RT_ERR_STATE, "%s: device %d does not hold mesh %d as the scene has it", who, D->device, mesh);
    DevMeshBufs &mb = D->mesh_bufs[mesh];
    hipStream_t st = D->stream;
    for (size_t i = 0; i < n_ev; i++) if (!ev[i].e) HIP_TRY(ev[i].create());
    const bool first = mb.vn.p == nullptr;
    const bool faces = with_faces && mb.fn.p == nullptr;      // (f alone may be there already: k_mesh_normals reads it too)
    const bool textured = mesh_textured(mb, m);
    // SMOOTH mode and no normals brought: the device computes them from the vertices it is about to be sent
    const bool smooth = m.normals_mode == RT_MESH_NORMALS_SMOOTH && !normals_changed;
    const bool posed = src == VERTICES_FROM_POSE;
    // a flagged pose on a device that has the positions: they become the previous ones where they are
    const bool swap_prev = posed && !m.v_prev.empty() && mb.v.p != nullptr;
    const bool upload_prev = src != VERTICES_ON_DEVICE && !m.v_prev.empty() && !swap_prev;
    if (swap_prev) std::swap(mb.v, mb.v_prev);
    if ((rs = mb.v.ensure(m.v.size() * 4)) || (rs = mb.vn.ensure(m.vn.size() * 4))) return rs;
    if (posed && (rs = prepare_mesh_pose(D, m, mb))) return rs;
    if (smooth && (rs = prepare_mesh_normals(D, m, mb))) return rs;
    // the store's normals are about to be read: never stale ones over what k_mesh_normals wrote here (the first time they are
    // the values the kernel's kept normals keep -- which stale ones are as well: a pose does not resolve the store for them)
    if ((first || normals_changed) && !(posed && smooth)) ensure_normals(m);
    // the previous positions follow the store: uploaded from it ahead of the new vertices, in the update's stream, by a flagged
    // update; released by an unflagged one (nothing is allocated, copied or freed for a mesh that never used the flag)
    if (upload_prev) { if (m.v_prev_stale) ensure_vertices(m); if ((rs = mb.v_prev.ensure(m.v_prev.size() * 4))) return rs; }
    else if (m.v_prev.empty() && src != VERTICES_ON_DEVICE) mb.v_prev.release();
    if (faces) {
        if ((rs = mb.f.ensure(m.f.size() * 4)) || (rs = mb.fn.ensure(m.fn.size() * 4))) return rs;
        if (textured && ((rs = mb.ft.ensure(m.ft.size() * 4)) || (rs = mb.vt.ensure(m.vt.size() * 4)))) return rs;
    }
    if (reserve && (rs = reserve())) return rs;
    HIP_TRY(hipEventRecord(ev[0], st));
    if (upload_prev) HIP_TRY(hipMemcpyAsync(mb.v_prev.p, m.v_prev.data(), m.v_prev.size() * 4, hipMemcpyHostToDevice, st));
    if (posed) { if ((rs = enqueue_mesh_pose(D, m, mb))) return rs; }
    else if (src == VERTICES_FROM_STORE) HIP_TRY(hipMemcpyAsync(mb.v.p, m.v.data(), m.v.size() * 4, hipMemcpyHostToDevice, st));
    if (first || normals_changed) HIP_TRY(hipMemcpyAsync(mb.vn.p, m.vn.data(), m.vn.size() * 4, hipMemcpyHostToDevice, st));
    if (faces) {
        HIP_TRY(hipMemcpyAsync(mb.f.p, m.f.data(), m.f.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(mb.fn.p, m.fn.data(), m.fn.size() * 4, hipMemcpyHostToDevice, st));
        if (textured) {
            HIP_TRY(hipMemcpyAsync(mb.ft.p, m.ft.data(), m.ft.size() * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(mb.vt.p, m.vt.data(), m.vt.size() * 4, hipMemcpyHostToDevice, st));
        }
    }
    if (smooth && (rs = enqueue_mesh_normals(D, m, mb))) return rs;      // k_mesh_retri, behind it in either tail, copies them into the slots
    HIP_TRY(hipEventRecord(ev[1], st));
    return RT_OK;
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

// ---- the refit -------------------------------------------------------------------------------------------------------------
// One device's share of a refitting update: everything upload_scene derived from this mesh's vertices, set again in place --
// DevTri and nrm of every slot and every box of the tree (rt_refit.hip), DevMesh::root_box, and the objects' cull boxes (objs: the
// scene's objects lowered again by the caller).  Nothing else on the device depends on a mesh's vertices: the tree's topology,
// stack_need (DevScene::max_bvh_depth, the spill buffers) and tex follow the faces, which stay.  quality (may be NULL): the
// refitted tree, measured behind the refit on the same stream.  box_for (NULL, or the scene of a pose no device has reported for
// yet): the host does not have the posed vertices, so m.root_box is read from the refitted tree's root record -- a second short
// synchronise -- and objs is lowered again from it, for this device and the ones after it.
static rt_status refit_mesh_on_device(DeviceState *D, rt::MeshData &m, int32_t mesh, bool normals_changed, std::vector<DevObject> &objs,
                                      rt_mesh_quality *quality, VertexSource src, const rt::SceneData *box_for)
{
    rt_status rs;
    if ((rs = begin_mesh_update(D, m, mesh, normals_changed, objs.size(), "rt_scene_update_mesh_vertices", D->upd_ev, 4, false, nullptr, src))) return rs;
    DevMeshBufs &mb = D->mesh_bufs[mesh];
    hipStream_t st = D->stream;
    MeshRefitRequest R = {};
    R.v = (const float *)mb.v.p; R.vn = (const float *)mb.vn.p;
    R.slot_idx = (const uint32_t *)mb.slot_idx.p; R.n_slots = (uint32_t)(m.f.size() / 3);
    R.tris = (DevTri *)mb.tris.p; R.nrm = (float *)mb.nrm.p; R.nodes = (DevBvhNode *)mb.nodes.p;
    R.level_nodes = (const uint32_t *)mb.level_nodes.p; R.level_off = mb.level_off.data(); R.n_levels = (int)mb.level_off.size() - 1;
    R.after_retri = D->upd_ev[2];
    HIP_TRY(rtk_launch_mesh_refit(st, R));
    HIP_TRY(hipEventRecord(D->upd_ev[3], st));
    D->upd_levels = R.n_levels;
    if (box_for) {
        HIP_TRY(hipMemcpyAsync(mb.root_rec_host, (const DevBvhNode *)mb.nodes.p + mb.root_ref, sizeof(DevBvhNode), hipMemcpyDeviceToHost, st));
        if (quality && (rs = enqueue_mesh_cost(D, mb))) return rs;
        HIP_TRY(hipStreamSynchronize(st));
        root_box_of_record(mb.root_rec_host, m.root_box);
        if ((rs = relower_objects(*box_for, objs))) return rs;
    }
    HIP_TRY(hipMemcpyAsync((char *)D->meshes.p + (size_t)mesh * sizeof(DevMesh) + offsetof(DevMesh, root_box), m.root_box, 24, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(D->objects.p, objs.data(), objs.size() * sizeof(DevObject), hipMemcpyHostToDevice, st));
    if (quality && !box_for && (rs = enqueue_mesh_cost(D, mb))) return rs;
    HIP_TRY(hipStreamSynchronize(st));
    return quality ? finish_mesh_cost(D, mb, quality) : RT_OK;
}

// ---- device tree build (rt_mi355x.h, "device tree build") ---------------------------------------------------------------------
// the host mirror: lbvh_build_host of rt_lbvh.h, the functions the kernels of rt_bvh_build.hip are made of in plain loops, behind the ABI's argument checks
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
    fill_device_bvh_info(info, bn.size(), faces.size(), root_ref, need);
    if (nodes && !bn.empty()) memcpy(nodes, bn.data(), bn.size() * sizeof(DevBvhNode));
    if (slot_face) memcpy(slot_face, faces.data(), faces.size() * 4);
    return RT_OK;
}

// the limit on a device-built tree's stack_need: what the kernels provide, or less under the test hook RT_LBVH_STACK_CAP (read at call time)
static int lbvh_stack_cap()
{
    int cap = RT_BVH_LDS + RT_BVH_SPILL;
    if (const char *e = getenv("RT_LBVH_STACK_CAP")) { const long v = strtol(e, nullptr, 10); if (v >= 0 && v < cap) cap = (int)v; }
    return cap;
}

// One device's share of a building update: the same upload, then the tree built from the vertices just uploaded
// (rt_bvh_build.hip) in place of the refit, the slots written in its order, and everything that follows a tree's topology set
// again -- the record count and DevMesh::nodes / root_ref, slot_face, level_off and level_nodes, stack_need with
// DevScene::max_bvh_depth and the spill buffers, built_cost.  Two host synchronisations: one for the record count, the levels and
// stack_need (the cost launch and the fallback decision need them), one at the end.
// *fell_back: the tree needs more stack than `cap`; the device is left for the caller to invalidate.  src and box_for: as in the
// refit -- here the root record comes with the first synchronise's copies, so a pose costs this tail no further one.
static rt_status build_mesh_on_device(DeviceState *D, rt::MeshData &m, int32_t mesh, bool normals_changed, std::vector<DevObject> &objs,
                                      int cap, rt_mesh_build_info *info, bool *fell_back, VertexSource src, const rt::SceneData *box_for)
{
    MeshBuildBufs &B = D->build;
    const size_t nf = m.f.size() / 3;
    const size_t sort_bytes = rtk_mesh_build_sort_bytes((uint32_t)nf);
    rt_status rs;
    // the scratch, and room for the records: fewer than nf (a record stands for a binary node with more than four keys beneath it)
    auto reserve = [&]() -> rt_status {
        DevMeshBufs &mb = D->mesh_bufs[mesh];
        const uint32_t blocks = (uint32_t)((nf + 255) / 256);
        rt_status r;
        if ((r = B.cbox.ensure(((size_t)blocks + 1) * 24)) || (r = B.keys[0].ensure(nf * 8)) || (r = B.keys[1].ensure(nf * 8)) || (r = B.sort_tmp.ensure(sort_bytes)) ||
            (r = B.bin.ensure(nf * sizeof(LbvhBin))) || (r = B.parent.ensure(nf * 4)) || (r = B.visit.ensure(nf * 4)) || (r = B.rec_bin.ensure(nf * 4)) ||
            (r = B.rec_held.ensure(nf * 4)) || (r = B.result.ensure(RT_LBVH_RESULT_WORDS * 4)) || (r = B.slot_face.ensure(nf * 4))) return r;
        if (nf > RT_LBVH_LEAF_TRIS && (r = mb.nodes.ensure(nf * sizeof(DevBvhNode)))) return r;      // (may move: DevMesh::nodes is set again below)
        return mb.level_nodes.ensure(nf * 4);
    };
    if ((rs = begin_mesh_update(D, m, mesh, normals_changed, objs.size(), "rt_scene_update_mesh_vertices_build", B.ev, 6, true, reserve, src))) return rs;
    DevMeshBufs &mb = D->mesh_bufs[mesh];
    hipStream_t st = D->stream;
    const bool textured = mesh_textured(mb, m);
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
    if (box_for) HIP_TRY(hipMemcpyAsync(mb.root_rec_host, mb.nodes.p, sizeof(DevBvhNode), hipMemcpyDeviceToHost, st));      // (record 0 is the root: the caller keeps a root leaf away)
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
    if (box_for) {
        root_box_of_record(mb.root_rec_host, m.root_box);
        if ((rs = relower_objects(*box_for, objs))) return rs;
    }
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

// ---- every device that holds the scene -------------------------------------------------------------------------------------
// step(D, objs, first, &stop) on every device that holds the scene, one after the other (caller holds s->mu, the store has the
// new vertices); objs: the scene's objects lowered again, once.  A device another call is using, or one the step fails on, lowers
// the scene again at its next use instead.  first: no device has succeeded yet -- every device holds the same tree (the same
// build, the same exact refit), so the first one that succeeds reports for all.  A step that sets stop is the last one: its
// device and every later one are invalidated as well (*stopped, if given, says that one did).  Returns the first error.
template <class Step> static rt_status on_devices_holding_scene(rt_scene *s, Step step, bool *stopped = nullptr)
{
    bool any = false, succeeded = false, stop = false;
    for (DeviceState *D : s->devs) any = any || D->scene_valid;
    if (!any) return RT_OK;
    std::vector<DevObject> objs;
    std::vector<DevObjectBack> backs;
    std::vector<int32_t> node_mat;
    const rt_status st = lower_objects(s->data, objs, backs, node_mat);
    int cur = 0;
    (void)hipGetDevice(&cur);
    rt_status ret = RT_OK;
    for (DeviceState *D : s->devs) {
        if (!D->scene_valid) continue;
        DeviceClaim claim(D);
        rt_status r = st;
        if (!r && claim.ok && !stop) {
            r = step(D, objs, !succeeded, &stop);      // (objs by reference: a pose's first step lowers them again)
            succeeded = succeeded || !r;
        }
        if (r || !claim.ok || stop) D->scene_valid = false;
        if (r && !ret) ret = r;
    }
    (void)hipSetDevice(cur);
    if (stopped) *stopped = stop;
    return ret;
}

// the refit on those devices.  quality: NULL, or where the first device that refits leaves the refitted tree's measure; flags
// RT_MESH_QUALITY_NOT_ON_DEVICE when none got as far (none holds the scene, all in use, or failed)
static rt_status refit_mesh_on_devices(rt_scene *s, int32_t mesh, bool normals_changed, rt_mesh_quality *quality, VertexSource src)
{
    if (quality) { quality->flags = RT_MESH_QUALITY_NOT_ON_DEVICE; quality->cost = quality->built_cost = 0.0; quality->ratio = 1.0; quality->measure_ms = 0.0f; }
    return on_devices_holding_scene(s, [&](DeviceState *D, std::vector<DevObject> &objs, bool first, bool *) {
        rt_mesh_quality mine = {};
        const bool measure = quality && first;
        const rt_status r = refit_mesh_on_device(D, s->data.meshes[mesh], mesh, normals_changed, objs, measure ? &mine : nullptr, src,
                                                 src == VERTICES_FROM_POSE && first ? &s->data : nullptr);
        if (!r && measure) { mine.struct_size = quality->struct_size; *quality = mine; }
        return r;
    });
}

// the device build on those devices.  info: the first building device's figures; flags ON_DEVICE, NOT_ON_DEVICE, or FELL_BACK -- a
// tree with stack_need above the limit.  The same mesh gives the same tree on every device: one that does not fit fits nowhere, no
// further device builds, and the call takes RT_MESH_UPDATE_REBUILD's path
static rt_status build_mesh_on_devices(rt_scene *s, int32_t mesh, bool normals_changed, rt_mesh_build_info *info, VertexSource src)
{
    const rt_mesh_build_info none = {sizeof(rt_mesh_build_info), RT_MESH_BUILD_NOT_ON_DEVICE};
    *info = none;
    const int cap = lbvh_stack_cap();
    bool fell_back = false;
    const rt_status ret = on_devices_holding_scene(s, [&](DeviceState *D, std::vector<DevObject> &objs, bool first, bool *stop) {
        rt_mesh_build_info mine = none;
        const rt_status r = build_mesh_on_device(D, s->data.meshes[mesh], mesh, normals_changed, objs, cap, &mine, stop, src,
                                                 src == VERTICES_FROM_POSE && first ? &s->data : nullptr);
        if (!r && first) { *info = mine; info->flags = *stop ? RT_MESH_BUILD_FELL_BACK : RT_MESH_BUILD_ON_DEVICE; }
        return r;
    }, &fell_back);
    if (fell_back) { s->invalidate(true, false); info->flags = RT_MESH_BUILD_FELL_BACK; }
    return ret;
}

// ---- the entry path --------------------------------------------------------------------------------------------------------
// what an entry point does once the store has the new vertices: refit; refit, measure, and take RT_MESH_UPDATE_REBUILD's path above
// max_ratio; build on the devices; or refit, measure, and build on the devices above max_ratio
enum UpdateAfter { UPDATE_REFIT, UPDATE_REFIT_MEASURE, UPDATE_BUILD, UPDATE_REFIT_MEASURE_BUILD };
// An entry point as the entry path sees it: its name for the messages, the flag bits it takes, whether max_ratio is an argument
// of it (the entry points it is one of word a refused flag their own way), and `after`.  The out-structs need no column: an
// entry point passes NULL for the one it does not have.
struct UpdateEntry { const char *who; uint32_t known; bool takes_ratio; UpdateAfter after; };
// every form there is, a row each, in EntryForm's order: six fed by vertices, and the same four fed by a bone pose and by a morph pose
enum EntryForm { ENTRY_VERTICES, ENTRY_VERTICES_FLAGS, ENTRY_VERTICES_AUTO, ENTRY_VERTICES_AUTO_FLAGS, ENTRY_VERTICES_BUILD, ENTRY_VERTICES_AUTO_BUILD,
                 ENTRY_POSE, ENTRY_POSE_AUTO, ENTRY_POSE_BUILD, ENTRY_POSE_AUTO_BUILD,
                 ENTRY_MORPH, ENTRY_MORPH_AUTO, ENTRY_MORPH_BUILD, ENTRY_MORPH_AUTO_BUILD, ENTRY_FORMS };
static const uint32_t FLAG_REBUILD = RT_MESH_UPDATE_REBUILD, FLAG_KEEP = RT_MESH_UPDATE_KEEP_PREVIOUS;
static const UpdateEntry ENTRIES[] = {
    // (takes what it always took: any bit but REBUILD stays RT_ERR_ARG, and the mesh holds no previous positions afterwards)
    {"rt_scene_update_mesh_vertices", FLAG_REBUILD, false, UPDATE_REFIT},
    {"rt_scene_update_mesh_vertices_flags", FLAG_REBUILD | FLAG_KEEP, false, UPDATE_REFIT},
    {"rt_scene_update_mesh_vertices_auto", 0u, true, UPDATE_REFIT_MEASURE},                    // (has no flags argument)
    {"rt_scene_update_mesh_vertices_auto_flags", FLAG_KEEP, true, UPDATE_REFIT_MEASURE},
    {"rt_scene_update_mesh_vertices_build", FLAG_KEEP, false, UPDATE_BUILD},
    {"rt_scene_update_mesh_vertices_auto_build", FLAG_KEEP, true, UPDATE_REFIT_MEASURE_BUILD},
    {"rt_scene_pose_mesh", FLAG_REBUILD | FLAG_KEEP, false, UPDATE_REFIT},
    {"rt_scene_pose_mesh_auto", FLAG_KEEP, true, UPDATE_REFIT_MEASURE},
    {"rt_scene_pose_mesh_build", FLAG_KEEP, false, UPDATE_BUILD},
    {"rt_scene_pose_mesh_auto_build", FLAG_KEEP, true, UPDATE_REFIT_MEASURE_BUILD},
    {"rt_scene_morph_mesh", FLAG_REBUILD | FLAG_KEEP, false, UPDATE_REFIT},
    {"rt_scene_morph_mesh_auto", FLAG_KEEP, true, UPDATE_REFIT_MEASURE},
    {"rt_scene_morph_mesh_build", FLAG_KEEP, false, UPDATE_BUILD},
    {"rt_scene_morph_mesh_auto_build", FLAG_KEEP, true, UPDATE_REFIT_MEASURE_BUILD},
};
static_assert(sizeof(ENTRIES) / sizeof(ENTRIES[0]) == ENTRY_FORMS, "a row for every EntryForm");

// A pose is computed on the devices unless the mesh's tree there is a single leaf -- no root record to read the box from; the mesh
// is tiny -- in which case the store resolves it now and the update goes the way of one that brought the vertices (caller holds s->mu)
static VertexSource pose_source(rt_scene *s, int32_t mesh)
{
    rt::MeshData &m = s->data.meshes[mesh];
    bool leaf = false;
    for (DeviceState *D : s->devs)
        if (D->scene_valid) leaf = leaf || m.f.size() / 3 <= RT_LBVH_LEAF_TRIS || ((size_t)mesh < D->mesh_bufs.size() && (D->mesh_bufs[mesh].root_ref & RT_COST_LEAF));
    if (!leaf) return VERTICES_FROM_POSE;
    ensure_vertices(m);
    return VERTICES_FROM_STORE;
}

static rt_status update_mesh_vertices(EntryForm form, rt_scene *s, int32_t mesh, const MeshInput &in, uint32_t flags, double max_ratio,
                                      rt_mesh_quality *q_out, rt_mesh_build_info *b_out)
{
    const UpdateEntry &e = ENTRIES[form];
    const bool pose = in.kind != INPUT_VERTICES;
    rt_status st = check_idle(s, e.who);
    if (st) return st;
    if (flags & ~e.known)
        return fail(RT_ERR_ARG, e.takes_ratio ? "%s: flag bits 0x%x (only RT_MESH_UPDATE_KEEP_PREVIOUS goes with max_ratio)" : "%s: unknown flag bits 0x%x", e.who, flags & ~e.known);
    if (e.takes_ratio && (!std::isfinite(max_ratio) || max_ratio < 1.0)) return fail(RT_ERR_ARG, "%s: max_ratio is %g (it must be finite and at least 1)", e.who, max_ratio);
    if (q_out && q_out->struct_size != sizeof(rt_mesh_quality))
        return fail(RT_ERR_ARG, "%s: rt_mesh_quality.struct_size is %u, this library's is %zu", e.who, q_out->struct_size, sizeof(rt_mesh_quality));
    if (b_out && b_out->struct_size != sizeof(rt_mesh_build_info))
        return fail(RT_ERR_ARG, "%s: rt_mesh_build_info.struct_size is %u, this library's is %zu", e.who, b_out->struct_size, sizeof(rt_mesh_build_info));
    if (!pose && !in.v) return fail(RT_ERR_ARG, "%s: v is NULL", e.who);
    std::lock_guard<std::mutex> lk(s->mu);
    const bool keep_previous = (flags & RT_MESH_UPDATE_KEEP_PREVIOUS) != 0;
    if ((st = pose ? store_mesh_pose(s, mesh, in, keep_previous, e.who) : store_mesh_vertices(s, mesh, in, keep_previous, e.who))) return st;
    if (flags & RT_MESH_UPDATE_REBUILD) { s->invalidate(true, false); return RT_OK; }      // (the next lowering uploads the previous positions from the store)
    const VertexSource src = pose ? pose_source(s, mesh) : VERTICES_FROM_STORE;
    const bool normals_changed = in.vn != nullptr, measure = e.after == UPDATE_REFIT_MEASURE || e.after == UPDATE_REFIT_MEASURE_BUILD;
    rt_mesh_quality q = {sizeof(rt_mesh_quality)};
    rt_mesh_build_info b = {sizeof(rt_mesh_build_info)};
    bool build = e.after == UPDATE_BUILD;
    if (!build) st = refit_mesh_on_devices(s, mesh, normals_changed, measure ? &q : nullptr, src);
    // a degenerate measure has ratio 1, and so has a scene no device holds: neither asks for a rebuild
    if (measure && !st && q.ratio > max_ratio) {
        q.flags |= RT_MESH_QUALITY_REBUILT;
        if (e.after == UPDATE_REFIT_MEASURE_BUILD) build = true; else s->invalidate(true, false);
    }
    // (behind a refit the vertices are on the devices already; the build sends them again with everything else it does, normals
    // only if this call brought some; a pose is not computed twice: its vertices stay where the refit's k_mesh_pose wrote them)
    if (build) st = build_mesh_on_devices(s, mesh, normals_changed, &b, src == VERTICES_FROM_POSE && e.after != UPDATE_BUILD ? VERTICES_ON_DEVICE : src);
    if (q_out) *q_out = q;
    if (b_out) *b_out = b;
    return st;
}

extern "C" rt_status rt_scene_update_mesh_vertices(rt_scene *s, int32_t mesh, const float *v, int32_t nv, const float *vn, int32_t nvn, uint32_t flags)
{
    return update_mesh_vertices(ENTRY_VERTICES, s, mesh, input_vertices(v, nv, vn, nvn), flags, 0.0, nullptr, nullptr);
}
extern "C" rt_status rt_scene_update_mesh_vertices_flags(rt_scene *s, int32_t mesh, const float *v, int32_t nv, const float *vn, int32_t nvn, uint32_t flags)
{
    return update_mesh_vertices(ENTRY_VERTICES_FLAGS, s, mesh, input_vertices(v, nv, vn, nvn), flags, 0.0, nullptr, nullptr);
}
extern "C" rt_status rt_scene_update_mesh_vertices_auto(rt_scene *s, int32_t mesh, const float *v, int32_t nv, const float *vn, int32_t nvn,
                                                        double max_ratio, rt_mesh_quality *out)
{
    return update_mesh_vertices(ENTRY_VERTICES_AUTO, s, mesh, input_vertices(v, nv, vn, nvn), 0u, max_ratio, out, nullptr);
}
extern "C" rt_status rt_scene_update_mesh_vertices_auto_flags(rt_scene *s, int32_t mesh, const float *v, int32_t nv, const float *vn, int32_t nvn,
                                                              double max_ratio, uint32_t flags, rt_mesh_quality *out)
{
    return update_mesh_vertices(ENTRY_VERTICES_AUTO_FLAGS, s, mesh, input_vertices(v, nv, vn, nvn), flags, max_ratio, out, nullptr);
}
extern "C" rt_status rt_scene_update_mesh_vertices_build(rt_scene *s, int32_t mesh, const float *v, int32_t nv, const float *vn, int32_t nvn,
                                                         uint32_t flags, rt_mesh_build_info *out)
{
    return update_mesh_vertices(ENTRY_VERTICES_BUILD, s, mesh, input_vertices(v, nv, vn, nvn), flags, 0.0, nullptr, out);
}
extern "C" rt_status rt_scene_update_mesh_vertices_auto_build(rt_scene *s, int32_t mesh, const float *v, int32_t nv, const float *vn, int32_t nvn,
                                                              double max_ratio, uint32_t flags, rt_mesh_quality *q_out, rt_mesh_build_info *out)
{
    return update_mesh_vertices(ENTRY_VERTICES_AUTO_BUILD, s, mesh, input_vertices(v, nv, vn, nvn), flags, max_ratio, q_out, out);
}

// the same four forms fed by a bone pose (rt_mi355x.h, "mesh skinning") ...
extern "C" rt_status rt_scene_pose_mesh(rt_scene *s, int32_t mesh, const float *bones, int32_t n_bones, uint32_t flags)
{
    return update_mesh_vertices(ENTRY_POSE, s, mesh, input_bones(bones, n_bones), flags, 0.0, nullptr, nullptr);
}
extern "C" rt_status rt_scene_pose_mesh_auto(rt_scene *s, int32_t mesh, const float *bones, int32_t n_bones, uint32_t flags, double max_ratio,
                                             rt_mesh_quality *out)
{
    return update_mesh_vertices(ENTRY_POSE_AUTO, s, mesh, input_bones(bones, n_bones), flags, max_ratio, out, nullptr);
}
extern "C" rt_status rt_scene_pose_mesh_build(rt_scene *s, int32_t mesh, const float *bones, int32_t n_bones, uint32_t flags, rt_mesh_build_info *out)
{
    return update_mesh_vertices(ENTRY_POSE_BUILD, s, mesh, input_bones(bones, n_bones), flags, 0.0, nullptr, out);
}
extern "C" rt_status rt_scene_pose_mesh_auto_build(rt_scene *s, int32_t mesh, const float *bones, int32_t n_bones, uint32_t flags, double max_ratio,
                                                   rt_mesh_quality *q_out, rt_mesh_build_info *out)
{
    return update_mesh_vertices(ENTRY_POSE_AUTO_BUILD, s, mesh, input_bones(bones, n_bones), flags, max_ratio, q_out, out);
}

// ... and by a morph pose (rt_mi355x.h, "morph targets"): weights, and bones that may be NULL with n_bones 0
extern "C" rt_status rt_scene_morph_mesh(rt_scene *s, int32_t mesh, const float *weights, int32_t n_targets, const float *bones, int32_t n_bones,
                                         uint32_t flags)
{
    return update_mesh_vertices(ENTRY_MORPH, s, mesh, input_morphs(weights, n_targets, bones, n_bones), flags, 0.0, nullptr, nullptr);
}
extern "C" rt_status rt_scene_morph_mesh_auto(rt_scene *s, int32_t mesh, const float *weights, int32_t n_targets, const float *bones, int32_t n_bones,
                                              uint32_t flags, double max_ratio, rt_mesh_quality *out)
{
    return update_mesh_vertices(ENTRY_MORPH_AUTO, s, mesh, input_morphs(weights, n_targets, bones, n_bones), flags, max_ratio, out, nullptr);
}
extern "C" rt_status rt_scene_morph_mesh_build(rt_scene *s, int32_t mesh, const float *weights, int32_t n_targets, const float *bones, int32_t n_bones,
                                               uint32_t flags, rt_mesh_build_info *out)
{
    return update_mesh_vertices(ENTRY_MORPH_BUILD, s, mesh, input_morphs(weights, n_targets, bones, n_bones), flags, 0.0, nullptr, out);
}
extern "C" rt_status rt_scene_morph_mesh_auto_build(rt_scene *s, int32_t mesh, const float *weights, int32_t n_targets, const float *bones,
                                                    int32_t n_bones, uint32_t flags, double max_ratio, rt_mesh_quality *q_out, rt_mesh_build_info *out)
{
    return update_mesh_vertices(ENTRY_MORPH_AUTO_BUILD, s, mesh, input_morphs(weights, n_targets, bones, n_bones), flags, max_ratio, q_out, out);
}

// ---- what the last update took ---------------------------------------------------------------------------------------------
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

// the last k_mesh_pose of one kind on a device (DeviceState::pose_ev): a bone pose's, or, morph, a morph pose's
static rt_status mesh_pose_ms(rt_scene *s, int device, float *ms, bool morph, const char *who, const char *never)
{
    if (!s || !ms) return fail(RT_ERR_ARG, "%s: NULL argument", who);
    DeviceState *D = find_device_state(s, device);
    if (!D || !D->pose_timed[morph]) return fail(RT_ERR_STATE, "%s: device %d has not %s a mesh", who, device, never);
    HIP_TRY(hipEventElapsedTime(ms, D->pose_ev[morph][0], D->pose_ev[morph][1]));
    return RT_OK;
}
extern "C" rt_status rt_scene_mesh_skin_ms(rt_scene *s, int device, float *ms) { return mesh_pose_ms(s, device, ms, false, "rt_scene_mesh_skin_ms", "posed"); }
extern "C" rt_status rt_scene_mesh_morph_ms(rt_scene *s, int device, float *ms) { return mesh_pose_ms(s, device, ms, true, "rt_scene_mesh_morph_ms", "morphed"); }

// ---- a mesh as it sits on a device ------------------------------------------------------------------------------------------
// What the three calls below share once their own arguments have passed: the mesh is one the scene has (*nv, if asked for: its
// vertex count), the scene is on `device` as it is now (lowered there first if need be), the device is claimed for the rest of
// the call -- `claim` is the caller's, to hold -- and an asynchronous render that may still be running there has been waited for.
static rt_status open_device_for_reading(rt_scene *s, int device, int32_t mesh, const char *who, DeviceState **D, std::optional<DeviceClaim> &claim,
                                         size_t *nv = nullptr)
{
    rt_status st;
    {
        std::lock_guard<std::mutex> lk(s->mu);
        if ((st = check_mesh_set(s, mesh, who))) return st;
        if (nv) *nv = s->data.meshes[mesh].v.size() / 3;
    }
    if ((st = prepare_device(s, device, D))) return st;
    claim.emplace(*D);
    if (!claim->ok) return fail(RT_ERR_STATE, "%s: another call on this scene is using device %d", who, device);
    if ((*D)->last_pending && (*D)->last_done) HIP_TRY(hipEventSynchronize((*D)->last_done));
    return RT_OK;
}

extern "C" rt_status rt_scene_mesh_quality(rt_scene *s, int device, int32_t mesh, rt_mesh_quality *out)
{
    if (!s || !out) return fail(RT_ERR_ARG, "rt_scene_mesh_quality: NULL argument");
    if (out->struct_size != sizeof(rt_mesh_quality))
        return fail(RT_ERR_ARG, "rt_scene_mesh_quality: rt_mesh_quality.struct_size is %u, this library's is %zu", out->struct_size, sizeof(rt_mesh_quality));
    DeviceState *D = nullptr;
    std::optional<DeviceClaim> claim;
    rt_status st = open_device_for_reading(s, device, mesh, "rt_scene_mesh_quality", &D, claim);
    if (st) return st;
    DevMeshBufs &mb = D->mesh_bufs[mesh];
    if ((st = enqueue_mesh_cost(D, mb))) return st;
    HIP_TRY(hipStreamSynchronize(D->stream));
    return finish_mesh_cost(D, mb, out);
}

extern "C" rt_status rt_scene_mesh_device_read(rt_scene *s, int device, int32_t mesh, rt_device_bvh_info *info, void *nodes, uint64_t nodes_cap,
                                               uint32_t *slot_face, uint64_t slots_cap, float *tris, float *nrm, float root_box[6])
{
    if (!s || !info) return fail(RT_ERR_ARG, "rt_scene_mesh_device_read: NULL argument");
    if (info->struct_size != sizeof(rt_device_bvh_info))
        return fail(RT_ERR_ARG, "rt_scene_mesh_device_read: rt_device_bvh_info.struct_size is %u, this library's is %zu", info->struct_size, sizeof(rt_device_bvh_info));
    DeviceState *D = nullptr;
    std::optional<DeviceClaim> claim;
    if (rt_status st = open_device_for_reading(s, device, mesh, "rt_scene_mesh_device_read", &D, claim)) return st;
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
    fill_device_bvh_info(info, n_nodes, n_slots, mb.root_ref, mb.stack_need);
    return RT_OK;
}

// the previous positions of one mesh as they sit on `device`, with rt_scene_mesh_device_read's discipline
extern "C" rt_status rt_scene_mesh_device_previous(rt_scene *s, int device, int32_t mesh, float *v_prev, uint64_t nv_cap, uint32_t *nv_out)
{
    if (!s || !nv_out) return fail(RT_ERR_ARG, "rt_scene_mesh_device_previous: NULL argument");
    DeviceState *D = nullptr;
    std::optional<DeviceClaim> claim;
    size_t nv = 0;
    if (rt_status st = open_device_for_reading(s, device, mesh, "rt_scene_mesh_device_previous", &D, claim, &nv)) return st;
    const DevMeshBufs &mb = D->mesh_bufs[mesh];
    if (!mb.v_prev.p) { *nv_out = 0; return RT_OK; }
    if (v_prev && nv_cap < nv) return fail(RT_ERR_ARG, "rt_scene_mesh_device_previous: room for %llu vertices, %zu needed", (unsigned long long)nv_cap, nv);
    HIP_TRY(hipStreamSynchronize(D->stream));
    if (v_prev) HIP_TRY(hipMemcpy(v_prev, mb.v_prev.p, nv * 12, hipMemcpyDeviceToHost));
    *nv_out = (uint32_t)nv;
    return RT_OK;
}
