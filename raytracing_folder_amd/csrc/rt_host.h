// rt_host.h -- private to the host files of the C ABI (not installed): what more than one of them needs.
//   rt_api.cpp     what needs no device state: errors, the scene store and its getters, the image and .dat wrappers
//   rt_lower.cpp   a scene onto a device (prepare_device): SAH BVH, objects, materials, textures
//   rt_mesh_update.cpp  a lowered mesh changed in place: the vertex-update entry points, refit, tree quality, device tree build,
//                  smooth normals, and the calls that read a mesh back from a device
//   rt_photons.cpp the photon maps: their setters, the gather structures (upload_photons), the photon and caustic passes,
//                  generate_photons, the global map's state (rt_photon_map.h) with its two device copies
//   rt_render.cpp  render orchestration: working sets, run_pipeline, render_tiles, the image-plane render entry points, the
//                  single-stage entry points
//   rt_exchange.cpp  the multi-GPU tile exchange: the packed layouts and their size queries, the packed render and the unpack
//                  entry points
//   rt_jobs.cpp    asynchronous jobs: the rt_render_begin* entry points, progress / stop / wait / statistics / destroy (struct
//                  rt_job itself is below: the orchestration of rt_render.cpp reads and writes it)
//   rt_post.cpp    the image-space stages (denoise .. motion blur)
// Everything here that has external linkage only so that these files can share it is hidden: the library's dynamic symbol
// table does not know it.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/rt_mi355x.h"
#include "host/rt_scene.h"
#include "rt_launch.h"
#include "rt_mesh_pose.h"
#include "rt_photon_map.h"

#define RT_HIDDEN __attribute__((visibility("hidden")))

// the message rt_last_error() returns: one thread-local, in rt_api.cpp
RT_HIDDEN rt_status fail(rt_status st, const char *fmt, ...);
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(RT_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

RT_HIDDEN bool device_is_gfx950(int dev);                              // rt_api.cpp
RT_HIDDEN void camera_setup(const rt_camera &cam, DevCamera &dc);      // of RenderPixel (rt_render.cpp)
// rt_scene_destroy of the last scene: the per-device scratch of the image-space stages goes with it (rt_post.cpp)
RT_HIDDEN void post_release_all();
// rt_post.cpp: an rt_scene_motion_device call that did not synchronise may still be reading the lowered scene on `device`; waited
// for on the host before that scene is overwritten (prepare_device, the in-place mesh update)
RT_HIDDEN rt_status motion_wait_host(int device);

struct DevBuf {
    void *p = nullptr; size_t bytes = 0;
    rt_status ensure(size_t n)
    {
        if (n <= bytes && p) return RT_OK;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        if (n == 0) n = 16;
        HIP_TRY(hipMalloc(&p, n));
        bytes = n;
        return RT_OK;
    }
    rt_status upload(const void *src, size_t n)
    {
        rt_status st = ensure(n);
        if (st) return st;
        if (n) HIP_TRY(hipMemcpy(p, src, n, hipMemcpyHostToDevice));
        return RT_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};
// a DevBuf released when its scope ends (DeviceState releases its own explicitly, on its device)
struct ScopedDevBuf : DevBuf {
    ScopedDevBuf() = default;
    ScopedDevBuf(const ScopedDevBuf &) = delete;
    ScopedDevBuf &operator=(const ScopedDevBuf &) = delete;
    ~ScopedDevBuf() { release(); }
};

// an owned hipEvent_t: destroyed with its owner, handed on by a move
struct RT_HIDDEN Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event &operator=(Event &&o) noexcept { std::swap(e, o.e); return *this; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e, flags); }      // once per Event
    operator hipEvent_t() const { return e; }
};

// ---- a scene on one device (rt_lower.cpp fills it, rt_mesh_update.cpp changes its meshes in place, rt_render.cpp renders from it) ----
// nodes .. tex are what DevMesh points to.  The rest serves rt_scene_update_mesh_vertices (rt_refit.hip) and is written at upload
// time with them: per triangle slot the three vertex and three normal indices of its face; the indices of the tree's nodes by
// depth, the deepest level first (level k is level_nodes[level_off[k] .. level_off[k + 1]), the root's level last); on the host,
// what rt_scene_mesh_device_read reports.  v and vn exist from the first update on.  v_prev: the mesh's previous positions
// (RT_MESH_UPDATE_KEEP_PREVIOUS; nv x 3 floats, indexed like v), there exactly while the store holds some: k_motion_mesh reads them.
struct DevMeshBufs {
    DevBuf nodes, tris, nrm, tex;
    DevBuf slot_idx, level_nodes, v, vn, v_prev;
    std::vector<uint32_t> level_off, slot_face;
    uint32_t root_ref = 0; int stack_need = 0;
    // mesh tree quality (rt_scene_mesh_quality): the cost of the tree as the host built it, from the host mirror on the host's own
    // records at upload time (no launch: the GPU's figure is the mirror's bit for bit) -- the only moment those records exist, and
    // after an update the store no longer has the vertices they were built for; k_bvh_cost's block sums on the device (from the
    // first measurement on) and where they land on the host: the block sums, then the root's 128-byte record as 16 doubles
    double built_cost = 0; uint32_t built_flags = 0;
    DevBuf cost_partials;
    std::vector<double> cost_host;
    // device tree build (rt_bvh_build.hip): the per-face index arrays and the texture vertices, on the device from the mesh's first build there
    DevBuf f, fn, ft, vt;
    // smooth normals (rt_mesh_normals.hip): the corners of every normal in CSR form, nadj_off[nvn + 1] and nadj_corner[3 nf] with the
    // corners of a row ascending, on the device from the mesh's first update in SMOOTH mode there (with f, which that kernel reads
    // too).  They follow the faces and fn, which stay: a device build keeps them.
    DevBuf nadj_off, nadj_corner;
    // mesh skinning (rt_mesh_pose.hip): the skin -- rest pose, bone indices, weights -- on the device from the mesh's first pose there
    // (skin_serial: which of the mesh's skins it is, MeshData::skin_serial), and the root record of the tree as a pose's tail reads it back
    DevBuf skin_rest, skin_index, skin_weight;
    uint32_t skin_serial = 0;
    float root_rec_host[32];
    void release_skin() { for (DevBuf *b : {&skin_rest, &skin_index, &skin_weight}) b->release(); }
    // morph targets (rt_mesh_pose.hip): the set -- base, deltas -- on the device from the mesh's first morph pose there
    // (morph_serial: MeshData::morph_serial)
    DevBuf morph_base, morph_deltas;
    uint32_t morph_serial = 0;
    void release_morphs() { morph_base.release(); morph_deltas.release(); }
    void release() { for (DevBuf *b : {&nodes, &tris, &nrm, &tex, &slot_idx, &level_nodes, &v, &vn, &v_prev, &cost_partials, &f, &fn, &ft, &vt, &nadj_off, &nadj_corner}) b->release(); release_skin(); release_morphs(); }
};
// the scratch of a device tree build (MeshBuildScratch of rt_launch.h), the device's own: grown to the largest mesh built there
struct MeshBuildBufs {
    DevBuf cbox, keys[2], sort_tmp, bin, parent, visit, rec_bin, rec_held, result, slot_face;
    std::vector<uint32_t> result_host, slot_face_host, level_nodes_host;
    Event ev[6];                        // between them: upload | keys + sort | hierarchy + boxes | collapse | slots + retri (the cost: DeviceState::cost_ev)
    void release() { for (DevBuf *b : {&cbox, &keys[0], &keys[1], &sort_tmp, &bin, &parent, &visit, &rec_bin, &rec_held, &result, &slot_face}) b->release(); for (Event &e : ev) e = Event(); }
};

static const size_t SPILL_BYTES = (size_t)RT_SPILL_BLOCKS * RT_BLOCK * RT_BVH_SPILL * 4;     // DevScene::bvh_spill / DevWork::bvh_spill

// Per-chunk working set.  A frame's chunks alternate between RT_STREAMS of these, each on its own HIP
// stream, so that the short launches of one chunk (deep bounce levels with few rays, whose duration is
// the latency of one ray's path) overlap the wide launches of the other.
#define RT_STREAMS 4                    /* slots compiled in; render_streams() says how many are used */
struct Workspace {
    DevBuf sample_rgb, sample_z, sample_hit, rq[2][5], pq[3], cq[3], counts, pixel_list;
    DevBuf bvh_spill;                   // traversal-stack entries beyond the kernels' LDS stacks (only for scenes whose BVHs can need them)
    DevBuf sample_fx;                   // reproducible renders only: 3 x int64 fixed-point secondary colour per sample (allocated on first use)
    DevBuf feat_second;                 // renders with feature planes only: one byte per chunk pixel, 1 = it took the second batch (k_mark_second)
    size_t samples = 0; uint32_t rq_cap = 0, pq_cap = 0;
    hipStream_t stream = nullptr;       // slot 0 runs on the caller's / the device's main stream instead
    void release()
    {
        for (DevBuf *b : {&sample_rgb, &sample_z, &sample_hit, &counts, &pixel_list, &bvh_spill, &sample_fx, &feat_second}) b->release();
        for (int i = 0; i < 2; i++) for (int k = 0; k < 5; k++) rq[i][k].release();
        for (int k = 0; k < 3; k++) { pq[k].release(); cq[k].release(); }
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
    }
};

// the device side of one photon map; what the kernels see of it is its DevPhotonMap (DeviceState::map pairs the two)
struct RT_HIDDEN PhotonStore {
    DevBuf pa, pb, box4, grid;          // the gather structure (rt_photon_build.hip)
    // per density-grid cell, the k-th squared distance of the last query k_gather answered there: predicts the next one's (a
    // hint that only steers which of two exact paths a query takes); zeroed whenever the structure is rebuilt
    DevBuf cell_rk2;
    int rk2_k = 0; float rk2_radius = 0;        // the gather parameters the hint table was filled under (0: empty)
    DevBuf cell_start;                  // DevPhotonMap::cell_start (built for the gather radius in use)
    bool valid = false;                 // the structure is the scene's map as it is now
    void release() { for (DevBuf *b : {&pa, &pb, &box4, &grid, &cell_rk2, &cell_start}) b->release(); }
};
struct PhotonMapRef { PhotonStore &store; DevPhotonMap &pm; };

struct DeviceState {
    int device = -1;
    bool scene_valid = false;
    DevBuf nodes, objects, objects_back, meshes, materials, material_class, lights, node_material, textures, texels, material_maps;
    std::vector<DevMeshBufs> mesh_bufs;
    std::vector<int32_t> node_object;           // per node: its object in the lowered scene (DevScene::objects), -1 when it carries none
    PhotonStore maps[2];                        // [0] the photon map (scene.pm), [1] the caustic map (scene.cm)
    DevBuf raw_photons;                         // 24-byte photons of the last photon pass on this device (1-based)
    DevBuf bvh_spill;                           // DevScene::bvh_spill of the single-stage entry points (rt_trace_rays, the photon pass); renders use their working set's
    DevScene scene{};
    Workspace ws[RT_STREAMS];
    DevBuf stats;
    std::atomic<int> busy{0};           // a host call is using the working sets of this device
    // an asynchronous render (sync == 0) returns while the GPU still uses the working sets, counters and
    // stats: `last_done` is recorded at its join and every later call orders its own stream behind it
    hipEvent_t last_done = nullptr;
    bool last_pending = false;
    bool last_pipelined = false;        // the render in flight ran every slot on the library's own streams (RenderAttempt::plan_chunks, fork_slots)
    uint64_t frame_seq = 0;             // rotates the slots from one pipelined frame to the next
    bool async_overflow = false;        // an asynchronous render dropped rays and nobody has collected that verdict yet (rt_render_check does)
    // How full the ray / photon-query queues of the last renders got, per sample of a chunk (device-side peaks,
    // rt_stats.peak_*): the next render of the same kind sizes its queues from that instead of the 2^bounce worst case
    // (choose_queue_sizing / record_queue_peaks in rt_render.cpp).
    struct QueueKey {                   // what makes two renders "of the same kind"
        int model = -1, bounce = -1, fan = -1; bool photons = false, caustic = false;
        bool operator==(const QueueKey &o) const { return model == o.model && bounce == o.bounce && fan == o.fan && photons == o.photons && caustic == o.caustic; }
    };
    struct QueueHistory { bool valid = false; QueueKey key; double rays_per_sample = 0, queries_per_sample = 0; } qhist;
    bool qhist_used = false;            // the render in flight (or last finished) was sized from qhist / the first-frame guess
    // scratch for the single-stage entry points
    DevBuf t_in, t_out[6];
    hipStream_t stream = nullptr;
    // the last in-place mesh update here (rt_scene_mesh_update_ms): events around its upload, k_mesh_retri and the refit launches
    Event upd_ev[4]; int upd_levels = -1;
    Event nrm_ev[2]; bool nrm_timed = false;        // around the last k_mesh_normals here (rt_scene_mesh_normals_ms)
    // around the last k_mesh_pose here of either kind: [0] a bone pose (rt_scene_mesh_skin_ms), [1] a morph pose, with or without
    // bones (rt_scene_mesh_morph_ms)
    Event pose_ev[2][2]; bool pose_timed[2] = {false, false};
    DevBuf skin_bones;                  // the bones k_mesh_pose stages from: 48 bytes a bone, uploaded at every pose that has any
    DevBuf morph_active;                // the active list k_mesh_pose reads: 8 bytes a non-zero weight, uploaded at every morph pose
    MeshMorphActive morph_active_host[RT_POSE_MAX_TARGETS];       // ... where the host compacts it (the source of an asynchronous copy)
    Event cost_ev[2];                   // around the last k_bvh_cost here and the copies behind it (rt_mesh_quality.measure_ms)
    MeshBuildBufs build;                // device tree builds here
    // one of the two maps: its buffers with what the kernels see of it
    PhotonMapRef map(bool caustic) { return {maps[caustic], caustic ? scene.cm : scene.pm}; }
    void release()
    {
        for (DevBuf *b : {&nodes, &objects, &objects_back, &meshes, &materials, &material_class, &lights, &node_material, &textures, &texels, &material_maps,
                          &raw_photons, &bvh_spill, &stats, &t_in}) b->release();
        for (PhotonStore &m : maps) m.release();
        for (auto &m : mesh_bufs) m.release();
        build.release();
        for (Event &e : upd_ev) e = Event();
        for (Event &e : cost_ev) e = Event();
        for (Event &e : nrm_ev) e = Event();
        nrm_timed = false;
        for (auto &kind : pose_ev) for (Event &e : kind) e = Event();
        pose_timed[0] = pose_timed[1] = false;
        skin_bones.release();
        morph_active.release();
        upd_levels = -1;
        for (Workspace &w : ws) w.release();
        for (int k = 0; k < 6; k++) t_out[k].release();
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
        if (last_done) (void)hipEventDestroy(last_done);
        last_done = nullptr; last_pending = false;
    }
};

// One host call at a time may use a device's working sets, scratch buffers, counters and stats: the render
// entry points AND the single-stage ones (rt_trace_rays, rt_shade_rays, rt_estimate_irradiance, rt_photon_pass)
// claim the device for their duration and fail with RT_ERR_STATE while another call (or a live job) holds it.
struct DeviceClaim {
    DeviceState *D; bool ok;
    explicit DeviceClaim(DeviceState *d) : D(d), ok(d->busy.exchange(1) == 0) {}
    ~DeviceClaim() { if (ok) D->busy.store(0); }
    DeviceClaim(const DeviceClaim &) = delete;
    DeviceClaim &operator=(const DeviceClaim &) = delete;
};

struct rt_scene {
    rt::SceneData data;
    GlobalPhotons global_photons;       // the global photon map: whose it is and where it lies (rt_photon_map.h); its balanced form is data.photons
    std::string photon_dump;            // where rt_render_begin's photon pass writes its .dat ("" = nowhere)
    std::mutex gen_mu;                  // jobs started together on several devices: ONE of them runs the photon pass, the others wait for it
    std::mutex mu;
    std::vector<DeviceState *> devs;
    std::atomic<int> live_jobs{0};
    std::atomic<uint32_t> render_flags{0};      // RT_RENDER_*: read once at the start of every render call
    void invalidate(bool scene, bool photons, bool caustic = false)
    {
        for (DeviceState *d : devs) { if (scene) d->scene_valid = false; if (photons) d->maps[0].valid = false; if (caustic) d->maps[1].valid = false; }
    }
    // a generated photon map is no longer this scene's (caller holds mu): gone, with the structures built from it
    void drop_generated_photons() { if (global_photons.drop_generated(data.photons)) invalidate(false, true); }
    // geometry, materials or lights changed (caller holds mu): re-upload, and a generated photon map was traced through the old ones
    void geometry_changed() { drop_generated_photons(); invalidate(true, false); }
};

// ---- what crosses the host files ----------------------------------------------------------------------------
RT_HIDDEN rt_status check_idle(rt_scene *s, const char *who);                                   // rt_api.cpp
// rt_api.cpp: the stored cyBVH arrays of a mesh, built again if a vertex update left them stale (caller holds s->mu)
RT_HIDDEN void ensure_reference_tree(rt::MeshData &m);
// rt_api.cpp: the stored normals of a mesh, computed again if an update in SMOOTH mode left them stale (caller holds s->mu); to
// be called wherever m.vn is read
RT_HIDDEN void ensure_normals(rt::MeshData &m);
// rt_api.cpp: the stored positions of a skinned mesh (and its previous positions, and root_box), computed again if a pose left them
// owed (caller holds s->mu); to be called wherever m.v or m.v_prev is read -- ensure_reference_tree and ensure_normals do
RT_HIDDEN void ensure_vertices(rt::MeshData &m);
// rt_api.cpp: RT_ERR_ARG unless every one of the pose's 12 n_bones floats is finite
RT_HIDDEN rt_status check_pose(const char *who, const float *bones, int32_t n_bones);
// rt_mesh_update.cpp: what the devices hold of one binding of a mesh -- its skin, or its morph set -- released (caller holds s->mu;
// the scene is idle)
enum MeshBinding { BINDING_SKIN, BINDING_MORPHS };
RT_HIDDEN void release_mesh_binding_on_devices(rt_scene *s, int32_t mesh, MeshBinding which);
// rt_api.cpp: RT_ERR_ARG unless `a` is there and every one of its n floats is finite (`what` names the array in the message)
RT_HIDDEN rt_status check_finite(const char *who, const char *what, const float *a, int64_t n);
// rt_api.cpp: RT_ERR_ARG "<who>: mesh <mesh> was never set" unless rt_scene_set_mesh has given the scene that mesh (caller holds s->mu)
RT_HIDDEN rt_status check_mesh_set(const rt_scene *s, int32_t mesh, const char *who);
// rt_lower.cpp: the scene's objects as upload_scene lowers them, with the material of every node; an in-place mesh update sends the
// objects again for their cull boxes (caller holds s->mu)
RT_HIDDEN rt_status lower_objects(const rt::SceneData &sd, std::vector<DevObject> &objs, std::vector<DevObjectBack> &backs, std::vector<int32_t> &node_mat);
// what every call that hands out a device tree says beside the records: its sizes, root and stack need, and the kernels' limits
inline void fill_device_bvh_info(rt_device_bvh_info *info, size_t n_nodes, size_t n_slots, uint32_t root_ref, int stack_need)
{
    info->n_nodes = (uint32_t)n_nodes; info->n_slots = (uint32_t)n_slots;
    info->root_ref = root_ref; info->stack_need = stack_need;
    info->bvh_lds = RT_BVH_LDS; info->bvh_stack = RT_BVH_STACK; info->bvh_spill = RT_BVH_SPILL;
    info->spill_blocks = RT_SPILL_BLOCKS; info->block = RT_BLOCK;
}
// rt_lower.cpp: the scene and both photon maps as they are now on `device`, under s->mu; the lookup alone (NULL: never prepared)
RT_HIDDEN rt_status prepare_device(rt_scene *s, int device, DeviceState **out);
RT_HIDDEN DeviceState *find_device_state(rt_scene *s, int device);
// rt_photons.cpp: the gather structure of one of the two maps on D (prepare_device calls it for a map that is not valid there,
// caller holds s->mu); the gather's cell table for a radius; generatePhotonMap as a whole
RT_HIDDEN rt_status upload_photons(rt_scene *s, DeviceState *D, bool caustic);
RT_HIDDEN rt_status ensure_cell_start(DeviceState *D, bool caustic, int k, float radius, hipStream_t st, bool *did_work = nullptr);
RT_HIDDEN rt_status generate_photons(rt_scene *s, int device, uint32_t max_photons, int photon_bounce, uint32_t seed, const char *dat_path,
                                     rt_setup_ms *ms_out, bool own_job);
RT_HIDDEN rt_status order_after_pending(DeviceState *D, hipStream_t st);                        // rt_render.cpp

// ---- render outputs (rt_render.cpp, rt_exchange.cpp, rt_jobs.cpp) -------------------------------------------
// The planes of rt_outputs in field order, with their bytes per pixel.  Internally a render's outputs are one Planes set
// indexed by this table; a NULL plane is not wanted, and nothing is allocated or launched for it.  PL_NORMAL .. PL_ID are the
// first-hit features (k_features).  PL_VARIANCE is not a field of rt_outputs (the struct cannot grow): it is the extra argument
// of the _var entry points, written by k_resolve's VAR instantiations.
enum Plane { PL_RGB8, PL_Z, PL_COUNT, PL_LINEAR, PL_NORMAL, PL_ALBEDO, PL_ALPHA, PL_ID, PL_VARIANCE, N_PLANES };
static const size_t PLANE_BYTES[N_PLANES] = {3, 4, 1, 12, 12, 12, 4, 4, 12};
struct Planes {
    void *p[N_PLANES] = {};
    Planes() = default;
    explicit Planes(const rt_outputs &o, float *variance = nullptr)
        : p{o.rgb8, o.z, o.count, o.rgb_linear, o.normal, o.albedo, o.alpha, o.object_id, variance} {}
    template <class T> T *at(int i) const { return (T *)p[i]; }
    DevFeatures features() const            // the planes k_features writes (rtk_launch_features)
    {
        DevFeatures f;
        f.normal = at<float>(PL_NORMAL); f.albedo = at<float>(PL_ALBEDO); f.alpha = at<float>(PL_ALPHA); f.object_id = at<int32_t>(PL_ID);
        return f;
    }
};
// the three planes of the entry points without a descriptor (the optional ones NULL but for rgb_linear)
inline rt_outputs outputs_of(uint8_t *rgb8, float *z, uint8_t *count, float *rgb_linear = nullptr)
{
    rt_outputs o = {(uint32_t)sizeof(rt_outputs), rgb8, z, count, rgb_linear};
    return o;
}
// rt_render.cpp: every entry point with image planes: the caller's sizeof first, then the three required planes
RT_HIDDEN rt_status check_outputs(const char *name, const rt_outputs *o);

// An asynchronous job.  rt_jobs.cpp starts, answers for and ends it; the struct is here because the orchestration reads and
// writes it while the job's thread renders (RenderAttempt in rt_render.cpp: stop and host read, progress and stats written).
struct rt_job {
    rt_scene *scene = nullptr;
    std::thread worker;
    std::atomic<int> progress{0};
    std::atomic<bool> stop{false};
    std::atomic<bool> done{false};
    rt_status status = RT_OK;
    std::string error;
    rt_stats stats{};
    // the caller-owned host planes (rt_render_begin*): finished bands are copied back chunk by chunk, so a
    // viewer that polls rt_render_progress can show the frame as it fills (viewport.cpp:367 reads
    // renderImage.GetPixels() while the workers run)
    Planes host;
    rt_setup_ms setup{};                // the photon pass this job ran first (all zero when it did not)
};

// What one render call writes, and how: image-sized device planes (`dev`; rgb_linear selects the linear plane, the features
// k_features), or packed records of the call's tiles (`packed`: rec_bytes 8, or 24 with the linear plane).  A strided job
// (rt_render_begin*, tile stride != 1) renders into packed records of rec_bytes and feature / variance staging planes of its own.
// Packed planes (rt_render_tiles_packed_outputs_device): `walk` names the sections of the caller's buffer behind the records --
// PL_NORMAL .. PL_VARIANCE, indexed by the call's tile walk like the records -- and packed_bytes is the whole contribution:
// what lies behind the records of the call's own tiles is zeroed in stream order before any kernel writes into it.
struct RenderRequest {
    Planes dev;
    void *packed = nullptr;
    size_t rec_bytes = 8;
    Planes walk;
    uint64_t packed_bytes = 0;          // packed planes only; 0: the packed entry points as they were
    hipStream_t stream = nullptr;       // the caller's stream; NULL: the device's own
    bool sync = true;
    rt_stats *stats_out = nullptr;
    rt_job *job = nullptr;
};
// rt_render.cpp: what every render call requires of its arguments, and the render itself -- what the entry points of all three
// files end in (a render whose history-sized queues overflowed is repeated once with worst-case queues)
RT_HIDDEN rt_status validate_render(const rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *t);
RT_HIDDEN rt_status render_tiles(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles, int device,
                                 const RenderRequest &req);
