// rt_photons.cpp -- the photon maps of a scene: their setters, the gather structure of each on a device (rt_photon_build.hip builds
// it; prepare_device in rt_lower.cpp asks for it through upload_photons), the photon and caustic passes, and generatePhotonMap as
// a whole.  The global map's state is rt_photon_map.h's GlobalPhotons; its two device copies are here.  rt_host.h is what the
// host files share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/rt_mi355x.h"
#include "host/rt_scene.h"
#include "rt_host.h"

// Gather structure of a photon map (rt_dev.h, built by rt_photon_build.hip on the GPU): the photons LocatePhotons can reach
// -- it descends only while index < halfStoredPhotons = n/2 - 1, cyPhotonMap.h:217,371, so heap slots >= 2*half are never
// visited: for a balanced array that is a prefix, for an unbalanced one everything but the `skip` indices -- re-sorted by
// recursive median splits into 2^D sub-leaves of <= RT_SUB_PHOTONS photons with their tight boxes; RT_LEAF_SUBS consecutive
// sub-leaves are one leaf (128 slots) of the tree the queries walk (boxes of all heap nodes in `box4`: the tree over the
// leaves is its head, the sub-leaf boxes its last level).  `src_dev` != NULL: the photons already sit on this device
// (n_src records, 0-based); else they are uploaded from `src_host`.  skip1: the records to leave out, ascending, counted from 1
// (the raw indices GlobalPhotons::skip keeps).
static rt_status build_photon_structure(DeviceState *D, bool caustic, const rt_photon *src_dev, const rt_photon *src_host, uint32_t n_src,
                                        const std::vector<uint32_t> &skip1, double *ms_upload = nullptr, double *ms_build = nullptr)
{
    using clk = std::chrono::steady_clock;
    auto [M, pm] = D->map(caustic);
    // nothing is published before the build and its final synchronisation have succeeded: a failure leaves the device WITHOUT a
    // valid map, so the next render tries again (and fails as loudly) instead of rendering without global illumination
    memset(&pm, 0, sizeof pm);
    M.valid = false;
    const uint32_t n_skip = (uint32_t)skip1.size();
    if (n_src <= n_skip) { M.valid = true; return RT_OK; }
    if (n_skip > 8) return fail(RT_ERR_LIMIT, "photon structure: %u photons to leave out, the device copy takes at most 8 (rt::UnreachablePhotons yields at most 4)", n_skip);
    const uint32_t n = n_src - n_skip;
    uint32_t n_leaves = 1;
    while ((size_t)n_leaves * RT_LEAF_SUBS * RT_SUB_PHOTONS < n) n_leaves <<= 1;
    // leaf ids travel as 16-bit values through the kernel's LDS lists; slots are addressed by 32-bit byte offsets
    if (n_leaves > 65536) return fail(RT_ERR_LIMIT, "photon map too large for the gather structure (%u photons, at most 8 Mi)", n);
    static_assert((65536ull * RT_LEAF_SUBS + 1) * RT_SUB_PHOTONS * sizeof(float4) <= 0xFFFFFFFFull, "photon slots are addressed by 32-bit byte offsets");
    const uint32_t n_sub = n_leaves * RT_LEAF_SUBS;
    rt_status st;
    hipStream_t stream = D->stream;
    const auto t0 = clk::now();
    ScopedDevBuf staged, compacted, scratch;
    const rt_photon *ph = src_dev;
    if (!ph) {
        if ((st = staged.ensure((size_t)n_src * sizeof(rt_photon)))) return st;
        HIP_TRY(hipMemcpyAsync(staged.p, src_host, (size_t)n_src * sizeof(rt_photon), hipMemcpyHostToDevice, stream));
        ph = (const rt_photon *)staged.p;
    }
    if (n_skip) {
        if ((st = compacted.ensure((size_t)n * sizeof(rt_photon)))) return st;
        uint32_t skip0[8];
        for (uint32_t k = 0; k < n_skip; k++) skip0[k] = skip1[k] - 1;
        rtk_photon_copy_skipping(stream, ph, n_src, skip0, n_skip, (rt_photon *)compacted.p);
        ph = (const rt_photon *)compacted.p;
    }
    HIP_TRY(hipStreamSynchronize(stream));
    const auto t1 = clk::now();
    // one more sub-leaf than the tree has, every slot empty: the kernel pads its sub-leaf lists with it
    const size_t slots = ((size_t)n_sub + 1) * RT_SUB_PHOTONS;
    const size_t sbytes = rtk_photon_structure_scratch(n, n_sub);
    if ((st = M.pa.ensure(slots * sizeof(float4))) || (st = M.pb.ensure(slots * sizeof(float4))) || (st = M.box4.ensure((size_t)4 * n_sub * sizeof(float4))) ||
        (st = M.grid.ensure((size_t)64 * 64 * 64 * 4)) || (st = scratch.ensure(sbytes))) return st;
    PhotonGridOut g;
    const hipError_t e = rtk_photon_structure(stream, ph, n, n_sub, (float4 *)M.pa.p, (float4 *)M.pb.p, (float4 *)M.box4.p, (uint32_t *)M.grid.p, &g, scratch.p, sbytes);
    hipError_t e2 = hipStreamSynchronize(stream);
    if (e != hipSuccess || e2 != hipSuccess) return fail(RT_ERR_DEVICE, "photon structure build failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    DevPhotonMap built;
    memset(&built, 0, sizeof built);
    built.pa = (const float4 *)M.pa.p; built.pb = (const float4 *)M.pb.p;
    built.tbox = (const float4 *)M.box4.p; built.sbox = (const float4 *)M.box4.p + 2 * (size_t)n_sub;
    built.n_leaves = n_leaves; built.n_photons = n;
    built.grid = (const uint32_t *)M.grid.p;
    for (int a = 0; a < 3; a++) { built.grid_min[a] = g.min[a]; built.grid_dim[a] = g.dim[a]; }
    built.cell = g.cell; built.inv_cell = 1.0f / g.cell;
    if ((st = M.cell_rk2.ensure((size_t)64 * 64 * 64 * 4))) return st;
    HIP_TRY(hipMemsetAsync(M.cell_rk2.p, 0, (size_t)64 * 64 * 64 * 4, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    pm = built;
    M.valid = true;
    M.rk2_k = 0;                                    // the hint table is empty: no gather parameters recorded yet
    const auto t2 = clk::now();
    if (ms_upload) *ms_upload += std::chrono::duration<double, std::milli>(t1 - t0).count();
    if (ms_build) *ms_build += std::chrono::duration<double, std::milli>(t2 - t1).count();
    return RT_OK;
}

// ---- the global map: its setters and its two device copies (caller holds s->mu) --------------------------------------
extern "C" rt_status rt_scene_set_photons(rt_scene *s, const rt_photon *photons, uint32_t n_stored)
{
    rt_status st = check_idle(s, "rt_scene_set_photons");
    if (st) return st;
    if (n_stored > 0 && !photons) return fail(RT_ERR_ARG, "rt_scene_set_photons: photons is NULL");
    std::lock_guard<std::mutex> lk(s->mu);
    s->global_photons.set_callers(s->data.photons, photons, n_stored);
    s->invalidate(false, true);
    return RT_OK;
}

extern "C" rt_status rt_scene_set_caustic_photons(rt_scene *s, const rt_photon *photons, uint32_t n_stored)
{
    rt_status st = check_idle(s, "rt_scene_set_caustic_photons");
    if (st) return st;
    if (n_stored > 0 && !photons) return fail(RT_ERR_ARG, "rt_scene_set_caustic_photons: photons is NULL");
    std::lock_guard<std::mutex> lk(s->mu);
    if (n_stored == 0) s->data.caustic_photons.clear();
    else s->data.caustic_photons.assign(photons, photons + (size_t)n_stored + 1);
    s->invalidate(false, false, true);
    return RT_OK;
}

// the generated photons on the host: copied from the device they lie on, once
static rt_status to_host(rt_scene *s)
{
    GlobalPhotons &g = s->global_photons;
    if (!g.host_copy_missing()) return RT_OK;
    const GlobalPhotons::DeviceSource src = g.source_on(g.device());        // the invariant: not on the host, so on a device
    int cur = 0;
    (void)hipGetDevice(&cur);
    HIP_TRY(hipSetDevice(g.device()->device));
    std::vector<rt_photon> raw((size_t)src.n + 1);
    HIP_TRY(hipMemcpy(raw.data(), src.photons, raw.size() * sizeof(rt_photon), hipMemcpyDeviceToHost));
    HIP_TRY(hipSetDevice(cur));
    g.set_host_copy(std::move(raw));
    return RT_OK;
}
// D->raw_photons is about to hold something else: a generated map that lies only there goes to the host first, and from here on
// the map is not on D, whatever a later build on D is told
static rt_status leaving_device(rt_scene *s, DeviceState *D)
{
    if (!s->global_photons.source_on(D)) return RT_OK;
    rt_status st = to_host(s);
    if (st) return st;
    s->global_photons.leave_device(D);
    return RT_OK;
}

rt_status upload_photons(rt_scene *s, DeviceState *D, bool caustic)
{
    const GlobalPhotons &g = s->global_photons;
    if (!caustic && g.is_generated()) {
        // as generated (unbalanced): everything but the photons balancing would put out of LocatePhotons' reach
        const GlobalPhotons::DeviceSource here = g.source_on(D);
        if (!here) {                                                             // another device: through the host
            rt_status st = to_host(s);
            if (st) return st;
            HIP_TRY(hipSetDevice(D->device));
        }
        return build_photon_structure(D, false, here ? here.photons + 1 : nullptr, here ? nullptr : g.host_raw().data() + 1, g.count(), g.skip());
    }
    const std::vector<rt_photon> &ph = caustic ? s->data.caustic_photons : s->data.photons;
    if (ph.size() < 2) { auto [M, pm] = D->map(caustic); memset(&pm, 0, sizeof(DevPhotonMap)); M.valid = true; return RT_OK; }
    const uint32_t n = (uint32_t)ph.size() - 1;
    return build_photon_structure(D, caustic, nullptr, ph.data() + 1, rt::ReachablePhotonSlots(n), {});
}

// DevPhotonMap::cell_start for the radius the gather is about to use: built on first use and again when a larger radius comes
// (a table built for a radius serves every smaller one), on the stream the gather will run on
rt_status ensure_cell_start(DeviceState *D, bool caustic, int k, float radius, hipStream_t st, bool *did_work)
{
    auto [M, pm] = D->map(caustic);
    // the per-cell k-th distances (PhotonStore::cell_rk2) are hints of ONE gather configuration: what queries with another k
    // or radius left there is dropped, so that it cannot steer this render's choice between the (exact) gather paths
    if (M.cell_rk2.p && M.rk2_k != 0 && (M.rk2_k != k || M.rk2_radius != radius)) {
        HIP_TRY(hipMemsetAsync(M.cell_rk2.p, 0, (size_t)64 * 64 * 64 * 4, st));
        if (did_work) *did_work = true;
    }
    M.rk2_k = k; M.rk2_radius = radius;
    if (pm.n_leaves < 2 || (pm.cell_start && radius <= pm.start_radius)) return RT_OK;
    rt_status s = M.cell_start.ensure((size_t)64 * 64 * 64 * 4);
    if (s) return s;
    rtk_photon_cell_start(st, pm.tbox, pm.n_leaves, pm.grid_min, pm.cell, pm.grid_dim, radius, (uint32_t *)M.cell_start.p);
    HIP_TRY(hipGetLastError());
    if (did_work) *did_work = true;
    pm.cell_start = (const uint32_t *)M.cell_start.p; pm.start_radius = radius;
    return RT_OK;
}

// ---- photon pass ----------------------------------------------------------------------------------------
// generatePhotonMap's two loops (P13/main.cpp:338-404): mode 0 = the photon map (stop when max_count photons are STORED),
// mode 1 = the caustic map (stop when max_count diffuse hits are COUNTED; only those behind more than one specular
// hit are stored).  Attempts are consumed in order, the count checked between attempts like the reference's while().
// Everything stays on the device: k_photon_trace writes each attempt's photons, rtk_photon_compact (rt_photon_build.hip)
// consumes the attempts in order and packs the stored photons into D->raw_photons (1-based, [0] zero), then
// ScalePhotonPowers.  The caller holds the device claim.
static rt_status photon_pass_device(rt_scene *s, DeviceState *D, uint32_t max_count, int photon_bounce, uint32_t seed, int mode,
                                    uint32_t *n_out, uint64_t *attempts_out, const char *who)
{
    if (max_count == 0 || photon_bounce < 1 || photon_bounce > 8) return fail(RT_ERR_ARG, "%s: need a positive count and 1 <= photon_bounce <= 8", who);
    if (max_count > (1u << 28)) return fail(RT_ERR_LIMIT, "%s: at most 2^28 photons", who);
    bool have_source = false;
    for (const rt_light &l : s->data.lights) if (l.type == RT_LIGHT_POINT) have_source = true;
    if (!have_source) return fail(RT_ERR_STATE, "%s: the scene has no photon source (point light)", who);
    rt_status st;
    {   // D->raw_photons is about to be overwritten
        std::lock_guard<std::mutex> lk(s->mu);
        if ((st = leaving_device(s, D))) return st;
    }
    const uint32_t batch = 1u << 18;
    static_assert((1u << 18) / RT_BLOCK <= RT_SPILL_BLOCKS, "DevScene::bvh_spill is sized for RT_SPILL_BLOCKS workgroups");
    const uint32_t out_cap = max_count + 8 + 1;                 // index 0 unused, up to 7 photons of overshoot
    if ((st = D->t_out[0].ensure((size_t)batch * 8 * 9 * 4))) return st;
    if ((st = D->t_out[1].ensure((size_t)batch * 4))) return st;
    if ((st = D->t_out[2].ensure(2 * sizeof(CompactState)))) return st;
    const size_t sbytes = rtk_photon_compact_scratch(batch);
    if ((st = D->t_out[3].ensure(sbytes))) return st;
    if ((st = D->raw_photons.ensure((size_t)out_cap * sizeof(rt_photon)))) return st;
    hipStream_t stream = D->stream;
    HIP_TRY(hipMemsetAsync(D->t_out[2].p, 0, 2 * sizeof(CompactState), stream));
    HIP_TRY(hipMemsetAsync(D->raw_photons.p, 0, sizeof(rt_photon), stream));
    CompactState h{0, 0, 0, 0};
    int empty_batches = 0;
    while (h.counted < max_count) {
        PhotonArgs pa = {};
        pa.first_attempt = h.attempts; pa.n_attempts = batch; pa.seed = seed; pa.max_bounce = photon_bounce; pa.mode = mode;
        pa.out = (float *)D->t_out[0].p; pa.count = (uint32_t *)D->t_out[1].p;
        rtk_launch_photon_trace(stream, D->scene, pa);
        rtk_photon_compact(stream, pa.out, pa.count, batch, mode, max_count, (CompactState *)D->t_out[2].p,
                           (rt_photon *)D->raw_photons.p, out_cap, D->t_out[3].p, sbytes);
        HIP_TRY(hipGetLastError());
        const unsigned long long before = h.counted;
        HIP_TRY(hipMemcpyAsync(&h, D->t_out[2].p, sizeof h, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (h.counted == before && ++empty_batches >= 4) return fail(RT_ERR_STATE, "%s: no photon is ever stored in this scene", who);
    }
    uint32_t n = h.stored;
    if (n + 1 > out_cap) n = out_cap - 1;
    if (n > 0) rtk_photon_scale(stream, (rt_photon *)D->raw_photons.p, n, (float)(1.0 * 4 * M_PI / n));      // ScalePhotonPowers(1.0*4*M_PI/NumPhotons), :366 / :400
    HIP_TRY(hipStreamSynchronize(stream));
    *n_out = n;
    if (attempts_out) *attempts_out = h.attempts;
    return RT_OK;
}

static rt_status photon_pass(rt_scene *s, int device, uint32_t max_count, int photon_bounce, uint32_t seed, int mode,
                             rt_photon *out, uint32_t out_cap, uint32_t *n_out, uint64_t *attempts_out, const char *who)
{
    if (!s || !out || !n_out) return fail(RT_ERR_ARG, "%s: NULL argument", who);
    if (max_count == 0 || photon_bounce < 1 || photon_bounce > 8) return fail(RT_ERR_ARG, "%s: need a positive count and 1 <= photon_bounce <= 8", who);
    if (out_cap < max_count + 8 + 1) return fail(RT_ERR_ARG, "%s: out must hold the count + 9 records (index 0 unused, up to 7 photons of overshoot)", who);
    DeviceState *D = nullptr;
    rt_status st = prepare_device(s, device, &D);
    if (st) return st;
    DeviceClaim claim(D);
    if (!claim.ok) return fail(RT_ERR_STATE, "%s: another call on this scene is using device %d", who, device);
    if ((st = order_after_pending(D, D->stream))) return st;
    uint32_t n = 0;
    if ((st = photon_pass_device(s, D, max_count, photon_bounce, seed, mode, &n, attempts_out, who))) return st;
    HIP_TRY(hipMemcpy(out, D->raw_photons.p, ((size_t)n + 1) * sizeof(rt_photon), hipMemcpyDeviceToHost));
    *n_out = n;
    return RT_OK;
}

extern "C" rt_status rt_photon_pass(rt_scene *s, int device, uint32_t max_photons, int photon_bounce, uint32_t seed,
                                    rt_photon *out, uint32_t out_cap, uint32_t *n_out, uint64_t *attempts_out)
{
    return photon_pass(s, device, max_photons, photon_bounce, seed, 0, out, out_cap, n_out, attempts_out, "rt_photon_pass");
}

extern "C" rt_status rt_caustic_pass(rt_scene *s, int device, uint32_t max_diffuse_hits, int photon_bounce, uint32_t seed,
                                     rt_photon *out, uint32_t out_cap, uint32_t *n_out, uint64_t *attempts_out)
{
    return photon_pass(s, device, max_diffuse_hits, photon_bounce, seed, 1, out, out_cap, n_out, attempts_out, "rt_caustic_pass");
}

// The device search (rt_photon_build.hip: photon_unreachable) for the photons of ph0 (as generated, 1-based, on the device) that
// balancing would put into heap slots reach + 1 .. n.  Three ways out: RT_OK with answered = true and their raw indices,
// ascending, in idx; RT_OK with answered = false when the search does not answer -- a median's key is not unique, the count does
// not come out, or the search is beyond its own level / segment limit -- and the host's replay has to; anything else when a runtime
// call or the scratch allocation failed.
static rt_status unreachable_on_device(hipStream_t stream, const rt_photon *ph0, uint32_t n, uint32_t reach, std::vector<uint32_t> &idx, bool &answered,
                                       const char *who)
{
    answered = false;
    ScopedDevBuf scratch;
    const size_t sbytes = rtk_photon_unreachable_scratch(n);
    rt_status st = scratch.ensure(sbytes);
    if (st) return st;
    uint32_t res[16];
    const hipError_t e = rtk_photon_unreachable(stream, ph0, n, reach + 1, n, scratch.p, sbytes, res);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "%s: the device search for unreachable photons failed: %s", who, hipGetErrorString(e));
    if (res[1] != 0 || res[0] != n - reach) return RT_OK;
    idx.assign(res + 2, res + 2 + res[0]);
    std::sort(idx.begin(), idx.end());
    answered = true;
    return RT_OK;
}

// generatePhotonMap as a whole (FIN/main.cpp:350-402).  `own_job`: called from the job thread of rt_render_begin (the scene
// counts that job as live; no other caller can be inside the scene then).
rt_status generate_photons(rt_scene *s, int device, uint32_t max_photons, int photon_bounce, uint32_t seed, const char *dat_path,
                           rt_setup_ms *ms_out, bool own_job)
{
    using clk = std::chrono::steady_clock;
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    if (!s) return fail(RT_ERR_ARG, "rt_scene_generate_photons: scene is NULL");
    rt_status st;
    if (!own_job && (st = check_idle(s, "rt_scene_generate_photons"))) return st;
    rt_setup_ms T;
    memset(&T, 0, sizeof T);
    const auto t_begin = clk::now();
    DeviceState *D = nullptr;
    if ((st = prepare_device(s, device, &D))) return st;
    DeviceClaim claim(D);
    if (!claim.ok) return fail(RT_ERR_STATE, "rt_scene_generate_photons: another call on this scene is using device %d", device);
    if ((st = order_after_pending(D, D->stream))) return st;
    if (D->last_pending && D->last_done) HIP_TRY(hipEventSynchronize(D->last_done));       // the structure is rebuilt in place
    {   // the map this call replaces: if it lives only on this device, it is simply dropped (not fetched to the host first)
        std::lock_guard<std::mutex> lk(s->mu);
        if (s->global_photons.host_copy_missing() && s->global_photons.device() == D) s->drop_generated_photons();
    }
    const auto t0 = clk::now();
    uint32_t n = 0;
    if ((st = photon_pass_device(s, D, max_photons, photon_bounce, seed, 0, &n, nullptr, "rt_scene_generate_photons"))) return st;
    const rt_photon *ph0 = (const rt_photon *)D->raw_photons.p;
    const auto t1 = clk::now();
    T.photon_pass = ms(t0, t1);
    // Which photons balancing would put out of LocatePhotons' reach (heap slots > ReachablePhotonSlots(n): the last three or four):
    // found ON THE DEVICE along the root paths of those slots (unreachable_on_device); the photons stay where they are.  They come
    // to the host only for the .dat dump, or when the device does not answer -- a median's key is not unique in its segment, as in
    // every map whose photons lie on axis-aligned walls: then the reference's swap sequence decides and the host replays it
    // (rt::UnreachablePhotons).
    std::vector<rt_photon> raw;
    const auto t2 = clk::now();
    if (dat_path && dat_path[0]) {
        raw.resize((size_t)n + 1);
        HIP_TRY(hipMemcpy(raw.data(), ph0, raw.size() * sizeof(rt_photon), hipMemcpyDeviceToHost));
        if ((st = rt_photons_write_dat(dat_path, raw.data(), n))) return st;
    }
    const auto t2b = clk::now();
    T.upload = ms(t2, t2b);
    std::vector<uint32_t> skip;
    const uint32_t reach = rt::ReachablePhotonSlots(n);
    if (n && reach < n) {
        bool answered = false;
        if (getenv("RT_UNREACHABLE_ON_HOST") == nullptr && (st = unreachable_on_device(D->stream, ph0, n, reach, skip, answered, "rt_scene_generate_photons"))) return st;
        if (!answered) {
            // the host's replay of BalanceSegment on (position, index) records packed on the device: 16 bytes per photon come over
            ScopedDevBuf packed;
            if ((st = packed.ensure(((size_t)n + 1) * 16))) return st;
            rtk_photon_pack_positions(D->stream, ph0, n, packed.p);
            std::vector<rt::PhotonPosRec> recs((size_t)n + 1);
            HIP_TRY(hipMemcpyAsync(recs.data(), packed.p, recs.size() * 16, hipMemcpyDeviceToHost, D->stream));
            HIP_TRY(hipStreamSynchronize(D->stream));
            rt::UnreachablePhotonRecs(recs.data(), n, skip);
        }
    }
    const auto t3 = clk::now();
    T.balance = ms(t2b, t3);
    double up = 0, build = 0;
    if ((st = build_photon_structure(D, false, ph0 + 1, nullptr, n, skip, &up, &build))) return st;
    T.upload += up; T.structure_build = build;
    {
        std::lock_guard<std::mutex> lk(s->mu);
        // raw: empty unless the photons had to come to the host
        s->global_photons.adopt_generated(s->data.photons, D, ph0, n, {max_photons, photon_bounce, seed}, std::move(skip), std::move(raw));
        for (DeviceState *d : s->devs) if (d != D) d->maps[0].valid = false;
    }
    T.total = ms(t_begin, clk::now());
    if (ms_out) *ms_out = T;
    return RT_OK;
}

extern "C" rt_status rt_scene_generate_photons(rt_scene *s, int device, uint32_t max_photons, int photon_bounce, uint32_t seed,
                                               const char *dat_path, rt_setup_ms *ms_out)
{
    return generate_photons(s, device, max_photons, photon_bounce, seed, dat_path, ms_out, false);
}

extern "C" rt_status rt_scene_set_photon_dump(rt_scene *s, const char *dat_path)
{
    rt_status st = check_idle(s, "rt_scene_set_photon_dump");
    if (st) return st;
    std::lock_guard<std::mutex> lk(s->mu);
    s->photon_dump = dat_path ? dat_path : "";
    return RT_OK;
}

extern "C" rt_status rt_scene_get_photons(rt_scene *s, rt_photon *out, uint32_t cap, uint32_t *n_stored)
{
    if (!s) return fail(RT_ERR_ARG, "rt_scene_get_photons: scene is NULL");
    std::lock_guard<std::mutex> lk(s->mu);
    const uint32_t n = s->global_photons.count();
    if (n_stored) *n_stored = n;
    if (!out) return RT_OK;
    if (cap < n + 1) return fail(RT_ERR_ARG, "rt_scene_get_photons: buffer of %u records, %u needed", cap, n + 1);
    if (n == 0) { memset(out, 0, sizeof(rt_photon)); return RT_OK; }
    if (s->global_photons.is_generated() && s->data.photons.empty()) {
        // PrepareForIrradianceEstimation (cyPhotonMap.h:196-218) of the generated photons, bit for bit, on first request
        if (rt_status st = to_host(s)) return st;
        std::vector<rt_photon> tmp = s->global_photons.host_raw();
        s->data.photons.resize(tmp.size());
        rt::BalancePhotons(tmp.data(), n, s->data.photons.data());
    }
    memcpy(out, s->data.photons.data(), ((size_t)n + 1) * sizeof(rt_photon));
    return RT_OK;
}

extern "C" rt_status rt_photon_unreachable_device(int device, const rt_photon *in, uint32_t n, uint32_t *raw_indices, uint32_t cap, uint32_t *count, int32_t *exact)
{
    if (!in || !count || !exact) return fail(RT_ERR_ARG, "rt_photon_unreachable_device: NULL argument");
    *count = 0; *exact = 1;
    if (!device_is_gfx950(device)) return fail(RT_ERR_NO_DEVICE, "rt_photon_unreachable_device: device %d is not gfx950 (no CPU path: rt_photon_unreachable is the host's)", device);
    const uint32_t reach = rt::ReachablePhotonSlots(n);
    if (n == 0 || reach >= n) return RT_OK;
    HIP_TRY(hipSetDevice(device));
    ScopedDevBuf ph;
    rt_status st;
    if ((st = ph.upload(in, ((size_t)n + 1) * sizeof(rt_photon)))) return st;
    HIP_TRY(hipMemset(ph.p, 0, sizeof(rt_photon)));                  // slot 0 is the unused all-zero photon
    std::vector<uint32_t> idx;
    bool answered = false;
    if ((st = unreachable_on_device(nullptr, (const rt_photon *)ph.p, n, reach, idx, answered, "rt_photon_unreachable_device"))) return st;
    if (!answered) { *exact = 0; return RT_OK; }
    *count = (uint32_t)idx.size();
    if (raw_indices) {
        if (cap < idx.size()) return fail(RT_ERR_ARG, "rt_photon_unreachable_device: room for %u indices, %zu needed", cap, idx.size());
        memcpy(raw_indices, idx.data(), idx.size() * 4);
    }
    return RT_OK;
}
