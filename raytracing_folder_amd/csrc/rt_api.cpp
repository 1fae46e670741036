// rt_api.cpp -- the part of the C ABI in include/rt_mi355x.h that needs no device state: errors, version, default parameters,
// the scene store and its getters, the image and .dat wrappers, the host-side BVH and photon helpers.
// Lowering a scene to the device layout of rt_dev.h is rt_lower.cpp, changing a lowered mesh in place rt_mesh_update.cpp (the
// store's part of a vertex update with it), the photon maps rt_photons.cpp, rendering rt_render.cpp, the image-space stages
// rt_post.cpp; rt_host.h is what they share.
// There is no CPU render path in this library: without a gfx950 device the render calls fail.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rt_mi355x.h"
#include "host/rt_scene.h"
#include "rt_host.h"
#include "rt_mesh_normals.h"
#include "rt_mesh_pose.h"
static_assert(RT_POSE_MAX_TARGETS == RT_MESH_MORPH_MAX_TARGETS, "rt_mesh_pose.h and rt_mi355x.h disagree on the target cap");

// ---- errors ---------------------------------------------------------------------------------------
static thread_local std::string g_err;       // the one message of rt_last_error(), whichever file failed
rt_status fail(rt_status st, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return st;
}

extern "C" const char *rt_last_error(void) { return g_err.c_str(); }
extern "C" int rt_abi_version(void) { return RT_ABI_VERSION; }

bool device_is_gfx950(int dev)
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return false;
    return strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

extern "C" int rt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    int ok = 0;
    for (int i = 0; i < n; i++) if (device_is_gfx950(i)) ok++;
    return ok;
}

extern "C" void rt_params_default(rt_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->min_sample = 4; p->max_sample = 8; p->threshold = 1e-3f; p->bounce = 4;      // FIN/main.cpp:19-26
    p->hemisphere_sample = 30; p->knn_k = 400; p->knn_radius = 1.0f;                // :26, :699
    p->shade_model = RT_SHADE_FIN; p->shadow_samples = 4; p->seed = 20171203u; p->gamma = 2.2;
    p->photon_count = 1000000; p->photon_bounce = 8;                                // MAX_NUM_OF_PHOTON, PHOTON_BOUNCE (:27, :29)
}

// ---- scene store ---------------------------------------------------------------------------------------
static std::atomic<int> g_live_scenes{0};
extern "C" rt_status rt_scene_create(rt_scene **out)
{
    if (!out) return fail(RT_ERR_ARG, "rt_scene_create: out is NULL");
    *out = new rt_scene;
    g_live_scenes.fetch_add(1);
    return RT_OK;
}

extern "C" void rt_scene_destroy(rt_scene *s)
{
    if (!s) return;
    // a job that is still rendering this scene holds a pointer to it: wait for it (jobs always terminate;
    // destroying the job first, or rt_render_stop, makes this immediate)
    while (s->live_jobs.load() > 0) std::this_thread::sleep_for(std::chrono::milliseconds(1));
    for (DeviceState *d : s->devs) {
        if (hipSetDevice(d->device) == hipSuccess) d->release();
        delete d;
    }
    delete s;
    if (g_live_scenes.fetch_sub(1) == 1) post_release_all();   // the last scene takes the per-device image-space scratch with it
}

rt_status check_idle(rt_scene *s, const char *who)
{
    if (!s) return fail(RT_ERR_ARG, "%s: scene is NULL", who);
    if (s->live_jobs.load() > 0) return fail(RT_ERR_STATE, "%s: a render job is still live on this scene", who);
    return RT_OK;
}

extern "C" rt_status rt_scene_set_render_flags(rt_scene *s, uint32_t flags)
{
    if (!s) return fail(RT_ERR_ARG, "rt_scene_set_render_flags: scene is NULL");
    const uint32_t known = RT_RENDER_REPRODUCIBLE | RT_RENDER_GENERAL_SHADING;
    if (flags & ~known) return fail(RT_ERR_ARG, "rt_scene_set_render_flags: unknown flag bits 0x%x", flags & ~known);
    rt_status st = check_idle(s, "rt_scene_set_render_flags");
    if (st) return st;
    std::lock_guard<std::mutex> lk(s->mu);
    // the material classes are part of the lowered scene: the next use of a device lowers it again (behind a render still in flight)
    if ((s->render_flags.load() ^ flags) & RT_RENDER_GENERAL_SHADING) s->invalidate(true, false);
    s->render_flags.store(flags);
    return RT_OK;
}

extern "C" rt_status rt_scene_get_render_flags(const rt_scene *s, uint32_t *flags)
{
    if (!s || !flags) return fail(RT_ERR_ARG, "rt_scene_get_render_flags: NULL argument");
    *flags = s->render_flags.load();
    return RT_OK;
}

extern "C" rt_status rt_scene_set_nodes(rt_scene *s, const rt_node *nodes, int32_t n)
{
    rt_status st = check_idle(s, "rt_scene_set_nodes");
    if (st) return st;
    if (n < 0 || (n > 0 && !nodes)) return fail(RT_ERR_ARG, "rt_scene_set_nodes: bad array");
    for (int32_t i = 0; i < n; i++) {
        if (i == 0 ? nodes[i].parent != -1 : (nodes[i].parent < 0 || nodes[i].parent >= i))
            return fail(RT_ERR_ARG, "rt_scene_set_nodes: node %d has parent %d (parents must precede children, root first)", i, nodes[i].parent);
        if (nodes[i].obj_type < RT_OBJ_NONE || nodes[i].obj_type > RT_OBJ_MESH)
            return fail(RT_ERR_ARG, "rt_scene_set_nodes: node %d has unknown object type %d", i, nodes[i].obj_type);
    }
    std::lock_guard<std::mutex> lk(s->mu);
    s->data.nodes.assign(nodes, nodes + n);
    s->geometry_changed();
    return RT_OK;
}

static void drop_mesh_skin(rt::MeshData &m), drop_mesh_morphs(rt::MeshData &m);
extern "C" rt_status rt_scene_set_mesh(rt_scene *s, int32_t mesh, const float *v, int32_t nv, const uint32_t *f, int32_t nf,
                                       const float *vn, int32_t nvn, const uint32_t *fn, const rt_bvh_node *nodes,
                                       int32_t nnodes, const uint32_t *elements)
{
    rt_status st = check_idle(s, "rt_scene_set_mesh");
    if (st) return st;
    if (mesh < 0 || mesh > 65535) return fail(RT_ERR_ARG, "rt_scene_set_mesh: mesh index %d out of range", mesh);
    if (nv <= 0 || nf <= 0 || nvn <= 0 || nnodes < 2 || !v || !f || !vn || !fn || !nodes || !elements)
        return fail(RT_ERR_ARG, "rt_scene_set_mesh: every array is required (nv=%d nf=%d nvn=%d nnodes=%d)", nv, nf, nvn, nnodes);
    for (int64_t i = 0; i < 3LL * nf; i++) {
        if (f[i] >= (uint32_t)nv) return fail(RT_ERR_ARG, "rt_scene_set_mesh: face index %u >= nv", f[i]);
        if (fn[i] >= (uint32_t)nvn) return fail(RT_ERR_ARG, "rt_scene_set_mesh: normal index %u >= nvn", fn[i]);
    }
    for (int32_t i = 0; i < nf; i++) if (elements[i] >= (uint32_t)nf) return fail(RT_ERR_ARG, "rt_scene_set_mesh: element %u >= nf", elements[i]);
    std::lock_guard<std::mutex> lk(s->mu);
    if ((size_t)mesh >= s->data.meshes.size()) s->data.meshes.resize((size_t)mesh + 1);
    rt::MeshData &m = s->data.meshes[mesh];
    m.v.assign(v, v + 3 * (size_t)nv); m.f.assign(f, f + 3 * (size_t)nf);
    m.vn.assign(vn, vn + 3 * (size_t)nvn); m.fn.assign(fn, fn + 3 * (size_t)nf);
    m.nodes.assign(nodes, nodes + nnodes); m.elements.assign(elements, elements + nf);
    m.tree_stale = false;
    m.vt.clear(); m.ft.clear();
    m.v_prev.clear();                   // the faces may have changed: no pairing of old and new vertices is vouched for
    m.normals_mode = RT_MESH_NORMALS_STORED; m.vn_stale = false;      // ... and the caller has just brought the normals it wants
    drop_mesh_skin(m);                  // ... and the vertex count may have: a skin is bound again by the caller
    drop_mesh_morphs(m);                // ... and so is a morph set
    s->geometry_changed();
    return RT_OK;
}

// A binding of a mesh dropped (its skin, its morph set), and with either what a pose left behind: nothing stays owed (the callers,
// s->mu held, have resolved v if the mesh is to keep its positions, so owed positions never outlive what they are owed from)
static void drop_mesh_poses(rt::MeshData &m) { m.pose = m.pose_prev = rt::MeshPose(); m.v_stale = m.v_prev_stale = false; }
static void drop_mesh_skin(rt::MeshData &m)
{
    m.skin_bones = 0;
    for (std::vector<float> *a : {&m.skin_weight, &m.skin_rest}) std::vector<float>().swap(*a);
    std::vector<uint16_t>().swap(m.skin_index);
    m.skin_serial++;
    drop_mesh_poses(m);
}
static void drop_mesh_morphs(rt::MeshData &m)
{
    m.morph_targets = 0;
    for (std::vector<float> *a : {&m.morph_base, &m.morph_deltas}) std::vector<float>().swap(*a);
    m.morph_serial++;
    drop_mesh_poses(m);
}
// positions a pose owes: mesh_pose_host over the base of the pose's kind -- a bone pose skins the skin's rest pose; a morph pose
// morphs the set's base and, if bones came with it, skins that
static void resolve_pose(const rt::MeshData &m, const rt::MeshPose &p, float *out)
{
    mesh_pose_host(p.morphed ? m.morph_base.data() : m.skin_rest.data(), m.v.size() / 3, m.morph_deltas.data(), p.morphed ? (uint32_t)m.morph_targets : 0u,
                   p.weights.data(), m.skin_index.data(), m.skin_weight.data(), p.bones.data(), p.skinned ? (uint32_t)m.skin_bones : 0u, out);
}
void ensure_vertices(rt::MeshData &m)
{
    if (m.v_prev_stale) resolve_pose(m, m.pose_prev, m.v_prev.data());
    m.v_prev_stale = false;
    if (!m.v_stale) return;
    resolve_pose(m, m.pose, m.v.data());
    rt::MeshRootBox(m.v.data(), m.f.data(), (unsigned)(m.f.size() / 3), m.root_box);
    m.v_stale = false;
}
void ensure_reference_tree(rt::MeshData &m)
{
    if (!m.tree_stale) return;
    ensure_vertices(m);
    rt::BuildMeanSplitBVH(m.v.data(), m.f.data(), (unsigned)(m.f.size() / 3), 4, m.nodes, m.elements);      // TriObj::Load's leaves of four
    m.tree_stale = false;
}
// the definition of "smooth normals" (rt_mi355x.h) on arrays whose indices have been checked: the adjacency, then every row
// walked by the function k_mesh_normals walks it with (rt_mesh_normals.h); vn holds the stored values and keeps those of the
// normals that have no corner or no direction
static void smooth_normals_host(const float *v, const uint32_t *f, const uint32_t *fn, size_t nf, size_t nvn, float *vn)
{
    std::vector<uint32_t> off(nvn + 1), corner(3 * nf);
    mesh_normal_adjacency(fn, nf, nvn, off.data(), corner.data());
    for (size_t j = 0; j < nvn; j++) {
        float n[3];
        if (mesh_smooth_normal(v, f, corner.data(), off[j], off[j + 1], n)) memcpy(vn + 3 * j, n, 12);
    }
}
void ensure_normals(rt::MeshData &m)
{
    if (!m.vn_stale) return;
    ensure_vertices(m);
    smooth_normals_host(m.v.data(), m.f.data(), m.fn.data(), m.f.size() / 3, m.vn.size() / 3, m.vn.data());
    m.vn_stale = false;
}
// for the getters, which take the scene const: the tree and, in SMOOTH mode, the normals are caches of what the vertices determine
static const rt::MeshData &mesh_with_tree(const rt_scene *s, int32_t mesh)
{
    rt_scene *w = const_cast<rt_scene *>(s);
    std::lock_guard<std::mutex> lk(w->mu);
    ensure_vertices(w->data.meshes[mesh]);
    ensure_reference_tree(w->data.meshes[mesh]);
    ensure_normals(w->data.meshes[mesh]);
    return w->data.meshes[mesh];
}

// the one answer to a mesh index nobody set (`who` names the entry point; caller holds s->mu)
rt_status check_mesh_set(const rt_scene *s, int32_t mesh, const char *who)
{
    if (mesh < 0 || (size_t)mesh >= s->data.meshes.size() || s->data.meshes[mesh].f.empty()) return fail(RT_ERR_ARG, "%s: mesh %d was never set", who, mesh);
    return RT_OK;
}

// ---- smooth normals (rt_mi355x.h, "smooth normals"; the kernel: rt_mesh_normals.hip, its launches: rt_mesh_update.cpp) ----------
extern "C" rt_status rt_mesh_smooth_normals(const float *v, int32_t nv, const uint32_t *f, const uint32_t *fn, int32_t nf, float *vn_inout, int32_t nvn)
{
    if (!v || !f || !vn_inout || nv <= 0 || nf <= 0 || nvn <= 0)
        return fail(RT_ERR_ARG, "rt_mesh_smooth_normals: v, f and vn_inout are required (nv=%d nf=%d nvn=%d)", nv, nf, nvn);
    if (!fn) fn = f;
    for (int64_t i = 0; i < 3LL * nf; i++) {
        if (f[i] >= (uint32_t)nv) return fail(RT_ERR_ARG, "rt_mesh_smooth_normals: face index %u >= nv", f[i]);
        if (fn[i] >= (uint32_t)nvn) return fail(RT_ERR_ARG, "rt_mesh_smooth_normals: normal index %u >= nvn", fn[i]);
    }
    smooth_normals_host(v, f, fn, (size_t)nf, (size_t)nvn, vn_inout);
    return RT_OK;
}

extern "C" rt_status rt_scene_set_mesh_normals_mode(rt_scene *s, int32_t mesh, uint32_t mode)
{
    rt_status st = check_idle(s, "rt_scene_set_mesh_normals_mode");
    if (st) return st;
    if (mode != RT_MESH_NORMALS_STORED && mode != RT_MESH_NORMALS_SMOOTH) return fail(RT_ERR_ARG, "rt_scene_set_mesh_normals_mode: unknown mode %u", mode);
    std::lock_guard<std::mutex> lk(s->mu);
    if ((st = check_mesh_set(s, mesh, "rt_scene_set_mesh_normals_mode"))) return st;
    rt::MeshData &m = s->data.meshes[mesh];
    // leaving SMOOTH: the normals the devices hold are those of the v of now, and a later update in STORED mode is to keep
    // exactly them -- the store's copy is brought up to date while it still has that v (no normal changes: a cache is filled)
    if (mode != RT_MESH_NORMALS_SMOOTH) ensure_normals(m);
    m.normals_mode = mode;
    return RT_OK;
}

extern "C" rt_status rt_scene_get_mesh_normals_mode(const rt_scene *s, int32_t mesh, uint32_t *mode)
{
    if (!s || !mode) return fail(RT_ERR_ARG, "rt_scene_get_mesh_normals_mode: NULL argument");
    std::lock_guard<std::mutex> lk(const_cast<rt_scene *>(s)->mu);
    if (rt_status st = check_mesh_set(s, mesh, "rt_scene_get_mesh_normals_mode")) return st;
    *mode = s->data.meshes[mesh].normals_mode;
    return RT_OK;
}

// ---- mesh skinning (rt_mi355x.h, "mesh skinning"; the kernel: rt_mesh_pose.hip, the pose entry points: rt_mesh_update.cpp) -----
// what the mirror and rt_scene_set_mesh_skin require of a skin (`who` names the entry point)
static rt_status check_skin(const char *who, int32_t n_bones, const uint16_t *bone_index, const float *weight, int32_t nv)
{
    if (!bone_index || !weight || nv <= 0) return fail(RT_ERR_ARG, "%s: bone_index and weight are required (nv=%d)", who, nv);
    if (n_bones < 1 || n_bones > RT_MESH_SKIN_MAX_BONES) return fail(RT_ERR_ARG, "%s: n_bones is %d (1 .. %d)", who, n_bones, RT_MESH_SKIN_MAX_BONES);
    for (int64_t i = 0; i < 4LL * nv; i++) {
        if (bone_index[i] >= n_bones) return fail(RT_ERR_ARG, "%s: vertex %lld names bone %u of %d", who, (long long)(i / 4), bone_index[i], n_bones);
        if (!std::isfinite(weight[i]) || weight[i] < 0.0f) return fail(RT_ERR_ARG, "%s: vertex %lld has weight %g (weights must be finite and >= 0)", who, (long long)(i / 4), weight[i]);
    }
    return RT_OK;
}
rt_status check_pose(const char *who, const float *bones, int32_t n_bones)
{
    if (!bones) return fail(RT_ERR_ARG, "%s: bones is NULL", who);
    for (int64_t i = 0; i < 12LL * n_bones; i++)
        if (!std::isfinite(bones[i])) return fail(RT_ERR_ARG, "%s: bone %lld has an entry that is not finite", who, (long long)(i / 12));
    return RT_OK;
}

extern "C" rt_status rt_mesh_skin(const float *v_rest, int32_t nv, const uint16_t *bone_index, const float *weight, const float *bones, int32_t n_bones,
                                  float *v_out)
{
    if (!v_rest || !v_out) return fail(RT_ERR_ARG, "rt_mesh_skin: v_rest and v_out are required");
    rt_status st = check_skin("rt_mesh_skin", n_bones, bone_index, weight, nv);
    if (st || (st = check_pose("rt_mesh_skin", bones, n_bones))) return st;
    mesh_skin_host(v_rest, (uint64_t)nv, bone_index, weight, bones, (uint32_t)n_bones, v_out);
    return RT_OK;
}

extern "C" rt_status rt_scene_set_mesh_skin(rt_scene *s, int32_t mesh, int32_t n_bones, const uint16_t *bone_index, const float *weight, int32_t nv)
{
    rt_status st = check_idle(s, "rt_scene_set_mesh_skin");
    if (st || (st = check_skin("rt_scene_set_mesh_skin", n_bones, bone_index, weight, nv))) return st;
    std::lock_guard<std::mutex> lk(s->mu);
    if ((st = check_mesh_set(s, mesh, "rt_scene_set_mesh_skin"))) return st;
    rt::MeshData &m = s->data.meshes[mesh];
    if ((size_t)nv != m.v.size() / 3) return fail(RT_ERR_ARG, "rt_scene_set_mesh_skin: nv is %d, the mesh has %zu vertices", nv, m.v.size() / 3);
    ensure_vertices(m);                 // the rest pose is the positions of now
    drop_mesh_skin(m);
    release_mesh_binding_on_devices(s, mesh, BINDING_SKIN);
    m.skin_bones = n_bones;
    m.skin_index.assign(bone_index, bone_index + 4 * (size_t)nv);
    m.skin_weight.assign(weight, weight + 4 * (size_t)nv);
    m.skin_rest = m.v;
    return RT_OK;
}

extern "C" rt_status rt_scene_clear_mesh_skin(rt_scene *s, int32_t mesh)
{
    rt_status st = check_idle(s, "rt_scene_clear_mesh_skin");
    if (st) return st;
    std::lock_guard<std::mutex> lk(s->mu);
    if ((st = check_mesh_set(s, mesh, "rt_scene_clear_mesh_skin"))) return st;
    rt::MeshData &m = s->data.meshes[mesh];
    ensure_vertices(m);                 // the mesh keeps the positions it has
    drop_mesh_skin(m);
    release_mesh_binding_on_devices(s, mesh, BINDING_SKIN);
    return RT_OK;
}

extern "C" rt_status rt_scene_mesh_skin_info(const rt_scene *s, int32_t mesh, rt_mesh_skin_info *out)
{
    if (!s || !out) return fail(RT_ERR_ARG, "rt_scene_mesh_skin_info: NULL argument");
    if (out->struct_size != sizeof(rt_mesh_skin_info))
        return fail(RT_ERR_ARG, "rt_scene_mesh_skin_info: rt_mesh_skin_info.struct_size is %u, this library's is %zu", out->struct_size, sizeof(rt_mesh_skin_info));
    std::lock_guard<std::mutex> lk(const_cast<rt_scene *>(s)->mu);
    if (rt_status st = check_mesh_set(s, mesh, "rt_scene_mesh_skin_info")) return st;
    const rt::MeshData &m = s->data.meshes[mesh];
    out->bound = m.skin_bones > 0;
    out->n_bones = m.skin_bones;
    out->nv = m.skin_bones > 0 ? (int32_t)(m.skin_rest.size() / 3) : 0;
    out->store_current = !m.v_stale;
    return RT_OK;
}

// ---- morph targets (rt_mi355x.h, "morph targets"; the kernel: rt_mesh_pose.hip, the pose entry points: rt_mesh_update.cpp) -----
// RT_ERR_ARG unless every one of n floats is finite (`what` names them)
rt_status check_finite(const char *who, const char *what, const float *a, int64_t n)
{
    if (!a) return fail(RT_ERR_ARG, "%s: %s is NULL", who, what);
    for (int64_t i = 0; i < n; i++)
        if (!std::isfinite(a[i])) return fail(RT_ERR_ARG, "%s: %s has an entry that is not finite (at %lld)", who, what, (long long)i);
    return RT_OK;
}
// what the mirror and rt_scene_set_mesh_morphs require of a set
static rt_status check_morphs(const char *who, int32_t n_targets, const float *deltas, int32_t nv)
{
    if (!deltas || nv <= 0) return fail(RT_ERR_ARG, "%s: deltas is required (nv=%d)", who, nv);
    if (n_targets < 1 || n_targets > RT_MESH_MORPH_MAX_TARGETS) return fail(RT_ERR_ARG, "%s: n_targets is %d (1 .. %d)", who, n_targets, RT_MESH_MORPH_MAX_TARGETS);
    return check_finite(who, "deltas", deltas, 3LL * nv * n_targets);
}

extern "C" rt_status rt_mesh_morph(const float *v_base, int32_t nv, const float *deltas, int32_t n_targets, const float *weights, float *v_out)
{
    if (!v_base || !v_out) return fail(RT_ERR_ARG, "rt_mesh_morph: v_base and v_out are required");
    rt_status st = check_morphs("rt_mesh_morph", n_targets, deltas, nv);
    if (st || (st = check_finite("rt_mesh_morph", "weights", weights, n_targets))) return st;
    mesh_morph_host(v_base, (uint64_t)nv, deltas, (uint32_t)n_targets, weights, v_out);
    return RT_OK;
}

extern "C" rt_status rt_scene_set_mesh_morphs(rt_scene *s, int32_t mesh, int32_t n_targets, const float *deltas, int32_t nv)
{
    rt_status st = check_idle(s, "rt_scene_set_mesh_morphs");
    if (st || (st = check_morphs("rt_scene_set_mesh_morphs", n_targets, deltas, nv))) return st;
    std::lock_guard<std::mutex> lk(s->mu);
    if ((st = check_mesh_set(s, mesh, "rt_scene_set_mesh_morphs"))) return st;
    rt::MeshData &m = s->data.meshes[mesh];
    if ((size_t)nv != m.v.size() / 3) return fail(RT_ERR_ARG, "rt_scene_set_mesh_morphs: nv is %d, the mesh has %zu vertices", nv, m.v.size() / 3);
    ensure_vertices(m);                 // the base is the positions of now
    drop_mesh_morphs(m);
    release_mesh_binding_on_devices(s, mesh, BINDING_MORPHS);
    m.morph_targets = n_targets;
    m.morph_deltas.assign(deltas, deltas + 3 * (size_t)nv * (size_t)n_targets);
    m.morph_base = m.v;
    return RT_OK;
}

extern "C" rt_status rt_scene_clear_mesh_morphs(rt_scene *s, int32_t mesh)
{
    rt_status st = check_idle(s, "rt_scene_clear_mesh_morphs");
    if (st) return st;
    std::lock_guard<std::mutex> lk(s->mu);
    if ((st = check_mesh_set(s, mesh, "rt_scene_clear_mesh_morphs"))) return st;
    rt::MeshData &m = s->data.meshes[mesh];
    ensure_vertices(m);                 // the mesh keeps the positions it has
    drop_mesh_morphs(m);
    release_mesh_binding_on_devices(s, mesh, BINDING_MORPHS);
    return RT_OK;
}

extern "C" rt_status rt_scene_mesh_morph_info(const rt_scene *s, int32_t mesh, rt_mesh_morph_info *out)
{
    if (!s || !out) return fail(RT_ERR_ARG, "rt_scene_mesh_morph_info: NULL argument");
    if (out->struct_size != sizeof(rt_mesh_morph_info))
        return fail(RT_ERR_ARG, "rt_scene_mesh_morph_info: rt_mesh_morph_info.struct_size is %u, this library's is %zu", out->struct_size, sizeof(rt_mesh_morph_info));
    std::lock_guard<std::mutex> lk(const_cast<rt_scene *>(s)->mu);
    if (rt_status st = check_mesh_set(s, mesh, "rt_scene_mesh_morph_info")) return st;
    const rt::MeshData &m = s->data.meshes[mesh];
    out->bound = m.morph_targets > 0;
    out->n_targets = m.morph_targets;
    out->nv = m.morph_targets > 0 ? (int32_t)(m.morph_base.size() / 3) : 0;
    out->store_current = !m.v_stale;
    return RT_OK;
}

// how many meshes of the scene hold previous positions, from the store (no device, no HIP call)
extern "C" rt_status rt_scene_previous_positions(const rt_scene *s, int32_t *n_meshes)
{
    if (!s || !n_meshes) return fail(RT_ERR_ARG, "rt_scene_previous_positions: NULL argument");
    std::lock_guard<std::mutex> lk(const_cast<rt_scene *>(s)->mu);
    int32_t n = 0;
    for (const rt::MeshData &m : s->data.meshes) n += !m.f.empty() && !m.v_prev.empty();
    *n_meshes = n;
    return RT_OK;
}


extern "C" rt_status rt_scene_set_mesh_texcoords(rt_scene *s, int32_t mesh, const float *vt, int32_t nvt, const uint32_t *ft)
{
    rt_status st = check_idle(s, "rt_scene_set_mesh_texcoords");
    if (st) return st;
    std::lock_guard<std::mutex> lk(s->mu);
    if (mesh < 0 || (size_t)mesh >= s->data.meshes.size() || s->data.meshes[mesh].f.empty())
        return fail(RT_ERR_ARG, "rt_scene_set_mesh_texcoords: mesh %d has not been set", mesh);
    rt::MeshData &m = s->data.meshes[mesh];
    if (nvt < 0 || (nvt > 0 && (!vt || !ft))) return fail(RT_ERR_ARG, "rt_scene_set_mesh_texcoords: bad arrays");
    for (size_t i = 0; nvt > 0 && i < m.f.size(); i++)
        if (ft[i] >= (uint32_t)nvt) return fail(RT_ERR_ARG, "rt_scene_set_mesh_texcoords: texture index %u >= nvt", ft[i]);
    if (nvt == 0) { m.vt.clear(); m.ft.clear(); }
    else { m.vt.assign(vt, vt + 3 * (size_t)nvt); m.ft.assign(ft, ft + m.f.size()); }
    s->invalidate(true, false);
    return RT_OK;
}

extern "C" rt_status rt_scene_get_mesh_texcoords(const rt_scene *s, int32_t mesh, int32_t *nvt, float *vt, uint32_t *ft)
{
    if (!s || mesh < 0 || (size_t)mesh >= s->data.meshes.size()) return fail(RT_ERR_ARG, "rt_scene_get_mesh_texcoords: bad mesh index");
    const rt::MeshData &m = s->data.meshes[mesh];
    if (nvt) *nvt = (int32_t)(m.vt.size() / 3);
    if (vt) memcpy(vt, m.vt.data(), m.vt.size() * 4);
    if (ft) memcpy(ft, m.ft.data(), m.ft.size() * 4);
    return RT_OK;
}

extern "C" rt_status rt_scene_set_materials(rt_scene *s, const rt_blinn *m, int32_t n)
{
    rt_status st = check_idle(s, "rt_scene_set_materials");
    if (st) return st;
    if (n < 0 || (n > 0 && !m)) return fail(RT_ERR_ARG, "rt_scene_set_materials: bad array");
    std::lock_guard<std::mutex> lk(s->mu);
    s->data.materials.assign(m, m + n);
    s->geometry_changed();
    return RT_OK;
}

extern "C" rt_status rt_scene_set_lights(rt_scene *s, const rt_light *l, int32_t n)
{
    rt_status st = check_idle(s, "rt_scene_set_lights");
    if (st) return st;
    if (n < 0 || (n > 0 && !l)) return fail(RT_ERR_ARG, "rt_scene_set_lights: bad array");
    for (int32_t i = 0; i < n; i++)
        if (l[i].type < RT_LIGHT_AMBIENT || l[i].type > RT_LIGHT_POINT) return fail(RT_ERR_ARG, "rt_scene_set_lights: light %d has unknown type", i);
    std::lock_guard<std::mutex> lk(s->mu);
    s->data.lights.assign(l, l + n);
    s->geometry_changed();
    return RT_OK;
}

extern "C" rt_status rt_scene_set_environment(rt_scene *s, const float env[3], const float bg[3])
{
    rt_status st = check_idle(s, "rt_scene_set_environment");
    if (st) return st;
    std::lock_guard<std::mutex> lk(s->mu);
    if (env) memcpy(s->data.env, env, 12);
    if (bg) memcpy(s->data.bg, bg, 12);
    s->invalidate(true, false);
    return RT_OK;
}

extern "C" rt_status rt_scene_get_environment(const rt_scene *s, float env[3], float bg[3])
{
    if (!s) return fail(RT_ERR_ARG, "rt_scene_get_environment: scene is NULL");
    if (env) memcpy(env, s->data.env, 12);
    if (bg) memcpy(bg, s->data.bg, 12);
    return RT_OK;
}

extern "C" rt_status rt_scene_set_textures(rt_scene *s, const rt_texture *tex, int32_t n, const uint8_t *texels, uint64_t n_bytes)
{
    rt_status st = check_idle(s, "rt_scene_set_textures");
    if (st) return st;
    if (n < 0 || (n > 0 && !tex) || (n_bytes > 0 && !texels)) return fail(RT_ERR_ARG, "rt_scene_set_textures: bad array");
    for (int32_t i = 0; i < n; i++) {
        if (tex[i].type != RT_TEX_FILE && tex[i].type != RT_TEX_CHECKER) return fail(RT_ERR_ARG, "rt_scene_set_textures: texture %d has unknown type", i);
        if (tex[i].type == RT_TEX_FILE && (tex[i].width < 0 || tex[i].height < 0 || (uint64_t)tex[i].texel_offset + 3ull * tex[i].width * tex[i].height > n_bytes))
            return fail(RT_ERR_ARG, "rt_scene_set_textures: texture %d exceeds the texel array", i);
    }
    std::lock_guard<std::mutex> lk(s->mu);
    s->data.textures.assign(tex, tex + n);
    s->data.texels.assign(texels, texels + n_bytes);
    s->invalidate(true, false);
    return RT_OK;
}

extern "C" rt_status rt_scene_set_material_maps(rt_scene *s, const rt_texmap *maps, int32_t n_materials)
{
    rt_status st = check_idle(s, "rt_scene_set_material_maps");
    if (st) return st;
    if (n_materials < 0 || (n_materials > 0 && !maps)) return fail(RT_ERR_ARG, "rt_scene_set_material_maps: bad array");
    std::lock_guard<std::mutex> lk(s->mu);
    s->data.material_maps.assign(maps, maps + 2 * (size_t)n_materials);
    s->invalidate(true, false);
    return RT_OK;
}

extern "C" rt_status rt_scene_set_environment_maps(rt_scene *s, const rt_texmap *environment, const rt_texmap *background)
{
    rt_status st = check_idle(s, "rt_scene_set_environment_maps");
    if (st) return st;
    std::lock_guard<std::mutex> lk(s->mu);
    rt_texmap none;
    memset(&none, 0, sizeof none);
    none.texture = RT_MAP_NONE;
    s->data.env_map = environment ? *environment : none;
    s->data.bg_map = background ? *background : none;
    s->invalidate(true, false);
    return RT_OK;
}

extern "C" rt_status rt_scene_get_textures(const rt_scene *s, rt_texture *tex, int32_t cap, uint8_t *texels, uint64_t texel_cap,
                                           int32_t *n_tex, uint64_t *n_bytes)
{
    if (!s) return fail(RT_ERR_ARG, "rt_scene_get_textures: scene is NULL");
    if (n_tex) *n_tex = (int32_t)s->data.textures.size();
    if (n_bytes) *n_bytes = s->data.texels.size();
    if (tex) { if ((size_t)cap < s->data.textures.size()) return fail(RT_ERR_ARG, "rt_scene_get_textures: capacity"); if (!s->data.textures.empty()) memcpy(tex, s->data.textures.data(), s->data.textures.size() * sizeof(rt_texture)); }
    if (texels) { if (texel_cap < s->data.texels.size()) return fail(RT_ERR_ARG, "rt_scene_get_textures: texel capacity"); if (!s->data.texels.empty()) memcpy(texels, s->data.texels.data(), s->data.texels.size()); }
    return RT_OK;
}

extern "C" rt_status rt_scene_get_maps(const rt_scene *s, rt_texmap *material_maps, int32_t cap, rt_texmap *environment, rt_texmap *background)
{
    if (!s) return fail(RT_ERR_ARG, "rt_scene_get_maps: scene is NULL");
    if (material_maps) {
        if ((size_t)cap < s->data.material_maps.size()) return fail(RT_ERR_ARG, "rt_scene_get_maps: capacity %d < %zu", cap, s->data.material_maps.size());
        if (!s->data.material_maps.empty()) memcpy(material_maps, s->data.material_maps.data(), s->data.material_maps.size() * sizeof(rt_texmap));
    }
    if (environment) *environment = s->data.env_map;
    if (background) *background = s->data.bg_map;
    return RT_OK;
}

extern "C" rt_status rt_image_read_rgb(const char *path, int32_t *w, int32_t *h, uint8_t *rgb, uint64_t cap)
{
    if (!path || !w || !h) return fail(RT_ERR_ARG, "rt_image_read_rgb: NULL argument");
    int iw = 0, ih = 0;
    std::vector<uint8_t> d;
    std::string err;
    if (!rt::ReadImageRGB(path, iw, ih, d, &err)) return fail(RT_ERR_IO, "rt_image_read_rgb(%s): %s", path, err.c_str());
    *w = iw; *h = ih;
    if (rgb) {
        if (cap < d.size()) return fail(RT_ERR_ARG, "rt_image_read_rgb: buffer of %llu bytes, need %zu", (unsigned long long)cap, d.size());
        memcpy(rgb, d.data(), d.size());
    }
    return RT_OK;
}

extern "C" rt_status rt_image_write_png(const char *path, const uint8_t *data, int32_t w, int32_t h, int32_t comps)
{
    if (!path || !data || w <= 0 || h <= 0) return fail(RT_ERR_ARG, "rt_image_write_png: bad argument");
    if (!rt::WritePNG(path, data, w, h, comps)) return fail(RT_ERR_IO, "rt_image_write_png(%s): cannot write (comps must be 1 or 3)", path);
    return RT_OK;
}

extern "C" rt_status rt_image_write_pfm(const char *path, const float *rgb, int32_t w, int32_t h)
{
    if (!path || !rgb || w <= 0 || h <= 0) return fail(RT_ERR_ARG, "rt_image_write_pfm: bad argument");
    if (!rt::WritePFM(path, rgb, w, h)) return fail(RT_ERR_IO, "rt_image_write_pfm(%s): cannot write", path);
    return RT_OK;
}

extern "C" rt_status rt_image_read_pfm(const char *path, int32_t *w, int32_t *h, float *rgb, uint64_t cap)
{
    if (!path || !w || !h) return fail(RT_ERR_ARG, "rt_image_read_pfm: NULL argument");
    int iw = 0, ih = 0;
    std::vector<float> d;
    std::string err;
    if (!rt::ReadPFM(path, iw, ih, d, &err)) return fail(RT_ERR_IO, "rt_image_read_pfm(%s): %s", path, err.c_str());
    *w = iw; *h = ih;
    if (rgb) {
        if (cap < d.size()) return fail(RT_ERR_ARG, "rt_image_read_pfm: room for %llu floats, need %zu", (unsigned long long)cap, d.size());
        memcpy(rgb, d.data(), d.size() * sizeof(float));
    }
    return RT_OK;
}

extern "C" rt_status rt_image_write_pfm1(const char *path, const float *v, int32_t w, int32_t h)
{
    if (!path || !v || w <= 0 || h <= 0) return fail(RT_ERR_ARG, "rt_image_write_pfm1: bad argument");
    if (!rt::WritePFM(path, v, w, h, 1)) return fail(RT_ERR_IO, "rt_image_write_pfm1(%s): cannot write", path);
    return RT_OK;
}

extern "C" rt_status rt_image_read_pfm1(const char *path, int32_t *w, int32_t *h, float *v, uint64_t cap)
{
    if (!path || !w || !h) return fail(RT_ERR_ARG, "rt_image_read_pfm1: NULL argument");
    int iw = 0, ih = 0;
    std::vector<float> d;
    std::string err;
    if (!rt::ReadPFM(path, iw, ih, d, &err, 1)) return fail(RT_ERR_IO, "rt_image_read_pfm1(%s): %s", path, err.c_str());
    *w = iw; *h = ih;
    if (v) {
        if (cap < d.size()) return fail(RT_ERR_ARG, "rt_image_read_pfm1: room for %llu floats, need %zu", (unsigned long long)cap, d.size());
        memcpy(v, d.data(), d.size() * sizeof(float));
    }
    return RT_OK;
}

extern "C" rt_status rt_image_zbuffer(const float *zbuffer, int32_t w, int32_t h, uint8_t *zbuffer_img)
{
    if (!zbuffer || !zbuffer_img || w <= 0 || h <= 0) return fail(RT_ERR_ARG, "rt_image_zbuffer: bad argument");
    rt::ZBufferImage(zbuffer, (size_t)w * (size_t)h, zbuffer_img);
    return RT_OK;
}

extern "C" rt_status rt_image_sample_count(const uint8_t *sample_count, int32_t w, int32_t h, uint8_t *sample_count_img, int32_t *smax)
{
    if (!sample_count || !sample_count_img || w <= 0 || h <= 0) return fail(RT_ERR_ARG, "rt_image_sample_count: bad argument");
    const int m = rt::SampleCountImage(sample_count, (size_t)w * (size_t)h, sample_count_img);
    if (smax) *smax = m;
    return RT_OK;
}

extern "C" rt_status rt_scene_load_xml(rt_scene *s, const char *path)
{
    rt_status st = check_idle(s, "rt_scene_load_xml");
    if (st) return st;
    if (!path) return fail(RT_ERR_ARG, "rt_scene_load_xml: path is NULL");
    rt::Scene graph;
    std::string err;
    if (!rt::LoadScene(graph, path, &err)) return fail(RT_ERR_IO, "rt_scene_load_xml(%s): %s", path, err.c_str());
    rt::SceneData d;
    if (!rt::Lower(graph, d, &err)) return fail(RT_ERR_ARG, "rt_scene_load_xml(%s): %s", path, err.c_str());
    std::lock_guard<std::mutex> lk(s->mu);
    if (!s->global_photons.is_generated()) d.photons = s->data.photons;      // a map the caller set stays; a generated one belonged to the old scene
    s->data = std::move(d);
    s->geometry_changed();
    return RT_OK;
}

extern "C" rt_status rt_scene_get_camera(const rt_scene *s, rt_camera *out)
{
    if (!s || !out) return fail(RT_ERR_ARG, "rt_scene_get_camera: NULL argument");
    if (!s->data.has_camera) return fail(RT_ERR_STATE, "rt_scene_get_camera: the scene has no camera (not loaded from XML)");
    *out = s->data.camera;
    return RT_OK;
}

extern "C" rt_status rt_scene_counts(const rt_scene *s, int32_t *n_nodes, int32_t *n_meshes, int32_t *n_materials,
                                     int32_t *n_lights, uint32_t *n_photons)
{
    if (!s) return fail(RT_ERR_ARG, "rt_scene_counts: scene is NULL");
    if (n_nodes) *n_nodes = (int32_t)s->data.nodes.size();
    if (n_meshes) *n_meshes = (int32_t)s->data.meshes.size();
    if (n_materials) *n_materials = (int32_t)s->data.materials.size();
    if (n_lights) *n_lights = (int32_t)s->data.lights.size();
    if (n_photons) *n_photons = s->global_photons.count();
    return RT_OK;
}

template <class T> static rt_status copy_out(const std::vector<T> &v, T *out, int32_t cap, const char *who)
{
    if (!out) return fail(RT_ERR_ARG, "%s: out is NULL", who);
    if ((size_t)cap < v.size()) return fail(RT_ERR_ARG, "%s: capacity %d < %zu", who, cap, v.size());
    if (!v.empty()) memcpy(out, v.data(), sizeof(T) * v.size());
    return RT_OK;
}
extern "C" rt_status rt_scene_get_nodes(const rt_scene *s, rt_node *out, int32_t cap) { return s ? copy_out(s->data.nodes, out, cap, "rt_scene_get_nodes") : fail(RT_ERR_ARG, "NULL scene"); }
extern "C" rt_status rt_scene_get_materials(const rt_scene *s, rt_blinn *out, int32_t cap) { return s ? copy_out(s->data.materials, out, cap, "rt_scene_get_materials") : fail(RT_ERR_ARG, "NULL scene"); }
extern "C" rt_status rt_scene_get_lights(const rt_scene *s, rt_light *out, int32_t cap) { return s ? copy_out(s->data.lights, out, cap, "rt_scene_get_lights") : fail(RT_ERR_ARG, "NULL scene"); }

extern "C" rt_status rt_scene_mesh_counts(const rt_scene *s, int32_t mesh, int32_t *nv, int32_t *nf, int32_t *nvn, int32_t *nnodes)
{
    if (!s || mesh < 0 || (size_t)mesh >= s->data.meshes.size()) return fail(RT_ERR_ARG, "rt_scene_mesh_counts: bad mesh index");
    const rt::MeshData &m = mesh_with_tree(s, mesh);
    if (nv) *nv = (int32_t)(m.v.size() / 3);
    if (nf) *nf = (int32_t)(m.f.size() / 3);
    if (nvn) *nvn = (int32_t)(m.vn.size() / 3);
    if (nnodes) *nnodes = (int32_t)m.nodes.size();
    return RT_OK;
}

extern "C" rt_status rt_scene_get_mesh(const rt_scene *s, int32_t mesh, float *v, uint32_t *f, float *vn, uint32_t *fn,
                                       rt_bvh_node *nodes, uint32_t *elements)
{
    if (!s || mesh < 0 || (size_t)mesh >= s->data.meshes.size()) return fail(RT_ERR_ARG, "rt_scene_get_mesh: bad mesh index");
    const rt::MeshData &m = mesh_with_tree(s, mesh);
    if (v) memcpy(v, m.v.data(), m.v.size() * 4);
    if (f) memcpy(f, m.f.data(), m.f.size() * 4);
    if (vn) memcpy(vn, m.vn.data(), m.vn.size() * 4);
    if (fn) memcpy(fn, m.fn.data(), m.fn.size() * 4);
    if (nodes) memcpy(nodes, m.nodes.data(), m.nodes.size() * sizeof(rt_bvh_node));
    if (elements) memcpy(elements, m.elements.data(), m.elements.size() * 4);
    return RT_OK;
}

extern "C" rt_status rt_bvh_build(const float *v, int32_t nv, const uint32_t *f, int32_t nf, int32_t max_per_leaf,
                                  rt_bvh_node *nodes_out, int32_t *nnodes, uint32_t *elements_out)
{
    if (!v || !f || nf <= 0 || nv <= 0 || !nodes_out || !nnodes || !elements_out) return fail(RT_ERR_ARG, "rt_bvh_build: NULL/empty argument");
    for (int64_t i = 0; i < 3LL * nf; i++) if (f[i] >= (uint32_t)nv) return fail(RT_ERR_ARG, "rt_bvh_build: face index out of range");
    std::vector<rt_bvh_node> nodes;
    std::vector<uint32_t> el;
    rt::BuildMeanSplitBVH(v, f, (unsigned)nf, (unsigned)max_per_leaf, nodes, el);
    memcpy(nodes_out, nodes.data(), nodes.size() * sizeof(rt_bvh_node));
    memcpy(elements_out, el.data(), el.size() * 4);
    *nnodes = (int32_t)nodes.size();
    return RT_OK;
}

extern "C" rt_status rt_photons_write_dat(const char *path, const rt_photon *photons, uint32_t n)
{
    if (!path || (n > 0 && !photons)) return fail(RT_ERR_ARG, "rt_photons_write_dat: NULL argument");
    FILE *fp = fopen(path, "wb");
    if (!fp) return fail(RT_ERR_IO, "rt_photons_write_dat: cannot create \"%s\"", path);
    const size_t w = n ? fwrite(photons + 1, sizeof(rt_photon), n, fp) : 0;
    const bool ok = (fclose(fp) == 0) && w == n;
    return ok ? RT_OK : fail(RT_ERR_IO, "rt_photons_write_dat: short write to \"%s\"", path);
}

extern "C" rt_status rt_photons_read_dat(const char *path, rt_photon *out, uint32_t cap, uint32_t *n)
{
    if (!path || !n) return fail(RT_ERR_ARG, "rt_photons_read_dat: NULL argument");
    FILE *fp = fopen(path, "rb");
    if (!fp) return fail(RT_ERR_IO, "rt_photons_read_dat: cannot open \"%s\"", path);
    fseek(fp, 0, SEEK_END);
    const long bytes = ftell(fp);
    rewind(fp);
    const uint64_t count = bytes > 0 ? (uint64_t)bytes / sizeof(rt_photon) : 0;
    if (count > 0xFFFFFFF0ull) { fclose(fp); return fail(RT_ERR_ARG, "rt_photons_read_dat: \"%s\" holds too many photons", path); }
    *n = (uint32_t)count;
    rt_status st = RT_OK;
    if (out) {
        if (cap < count + 1) st = fail(RT_ERR_ARG, "rt_photons_read_dat: buffer of %u records, %llu needed", cap, (unsigned long long)count + 1);
        else {
            memset(out, 0, sizeof(rt_photon));
            if (count && fread(out + 1, sizeof(rt_photon), count, fp) != count) st = fail(RT_ERR_IO, "rt_photons_read_dat: short read from \"%s\"", path);
        }
    }
    fclose(fp);
    return st;
}

extern "C" rt_status rt_photon_balance(rt_photon *in, uint32_t n, rt_photon *out)
{
    if (!in || !out) return fail(RT_ERR_ARG, "rt_photon_balance: NULL argument");
    rt::BalancePhotons(in, n, out);
    return RT_OK;
}

extern "C" rt_status rt_photon_unreachable(const rt_photon *in, uint32_t n, uint32_t *raw_indices, uint32_t cap, uint32_t *count)
{
    if (!in || !count) return fail(RT_ERR_ARG, "rt_photon_unreachable: NULL argument");
    std::vector<uint32_t> idx;
    rt::UnreachablePhotons(in, n, idx);
    *count = (uint32_t)idx.size();
    if (raw_indices) {
        if (cap < idx.size()) return fail(RT_ERR_ARG, "rt_photon_unreachable: room for %u indices, %zu needed", cap, idx.size());
        if (!idx.empty()) memcpy(raw_indices, idx.data(), idx.size() * 4);
    }
    return RT_OK;
}
