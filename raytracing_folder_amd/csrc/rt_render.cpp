// rt_render.cpp -- rendering from a prepared device (rt_lower.cpp): per-chunk wavefront orchestration on HIP streams behind
// render_tiles, the image-plane render entry points of the C ABI in include/rt_mi355x.h, rt_render_check / rt_render_counters, and
// the single-stage entry points.  The tile exchange (rt_exchange.cpp) and the asynchronous jobs (rt_jobs.cpp) render through
// render_tiles.  rt_host.h is what the host files share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/rt_mi355x.h"
#include "host/rt_scene.h"
#include "rt_host.h"

// k_gather is a persistent grid that pulls query batches from a counter: enough workgroups to fill
// every CU at the kernel's occupancy (256 CUs x 5 resident workgroups of 4 waves)
static int gather_blocks()
{
    static int n = 0;
    if (n == 0) {
        const char *e = getenv("RT_GATHER_BLOCKS");     // tuning experiments only
        const long v = e ? atol(e) : 0;
        n = (v >= 64 && v <= 16384) ? (int)v : 256 * 5;
    }
    return n;
}
static const size_t STATS_BYTES = (size_t)ST_COUNT * RT_STAT_STRIDE * 8;    // the statistics block: counters RT_STAT_STRIDE apart (rt_dev.h)

// Queue sizing policy: the first render of a kind (shading model, bounce limit, fan-out, maps in use) provides one ray and
// half a photon query per sample, later ones twice what the fullest chunk so far needed (at least 1 ray and 0.25 queries per sample);
// if that ever overflows, a synchronous render
// is repeated once with the worst-case size (2^bounce per sample) -- an asynchronous one cannot be repeated by the
// library: it starts from the worst case unless there is history, and an overflow is reported by rt_render_check.
struct QueueSizing {
    DeviceState::QueueKey key;
    bool hist_ok = false;                       // the device's history is of this kind of render
    double ray_factor = 0, query_factor = 0;    // queue entries per sample to provide (ensure_workspace); 0 = worst case
};
// The factors for the render that is about to start; can_retry: the library itself can render it again when they prove too small.
static QueueSizing choose_queue_sizing(DeviceState *D, const rt_params &p, bool worst_case, bool can_retry)
{
    QueueSizing q;
    q.key.model = p.shade_model; q.key.bounce = p.bounce;
    // P12: a diffuse hit spawns hemisphere rays on top of the reflection/refraction pair; in practice one
    // of the three classes dominates per material, so the queues are sized for a fan-out of 2 and an
    // overflow is reported as an error rather than silently dropped
    q.key.fan = p.shade_model == RT_SHADE_P12 && p.hemisphere_sample > 1 ? 1 + p.hemisphere_sample : 2;
    q.key.photons = D->scene.pm.n_leaves != 0; q.key.caustic = p.caustic_k > 0 && D->scene.cm.n_leaves != 0;
    const DeviceState::QueueHistory &H = D->qhist;
    q.hist_ok = H.valid && H.key == q.key;
    if (!worst_case && getenv("RT_QUEUE_WORST_CASE") == nullptr) {
        // floors: how many rays k_wavefront cannot keep in LDS depends on timing, and a view change can bring glass into a
        // frame that had none -- one ray (160 B of queue) and a quarter of a query (12 B) per sample: 1.4 GB per 8 Mi-sample working
        // set of a job, 11.5 GB per 64 Mi-sample one of a device-side render -- and cover both
        if (q.hist_ok) { q.ray_factor = std::max(2.0 * H.rays_per_sample, 1.0); q.query_factor = std::max(2.0 * H.queries_per_sample, 0.25); }
        else if (can_retry) {
            // first render of a kind: from the model's fan-out.  k_wavefront keeps the ray tree in LDS (the global queue only sees
            // what does not fit).  The per-level models put a whole level into the queue: about one hemisphere ray per path that
            // is still alive (P12: hemisphere_sample of them on the first level, RayTracingProj12 main.cpp:393-446) PLUS the
            // ungated reflection / refraction pairs of the P13-family Shade, which double level by level inside glass
            // (P13/main.cpp:633-751: measured 2.5 rays per sample on the fullest level of a Cornell chunk that holds the glass
            // sphere, bounce 8) -- four per sample on top of the hemisphere rays, 640 B per sample of queue memory
            // (the kernels' own predicate: a scene k_wavefront does not take -- a BVH beyond its traversal stack, RT_TRACER=levels -- goes
            // through the per-level kernels and gets their figure; P12 through k_wavefront keeps the per-level figure too: its overflow is scene-dependent)
            const bool wf = rtk_wavefront_usable(D->scene, p) && p.shade_model != RT_SHADE_P12;
            q.ray_factor = wf ? 1.0 : (p.shade_model == RT_SHADE_P12 ? (double)std::max(p.hemisphere_sample, 1) + 3.0 : 4.0);
            q.query_factor = 0.5;
        }
    }
    D->qhist_used = q.ray_factor > 0 || q.query_factor > 0;
    return q;
}
// The peaks of a render that finished without a drop, per sample of a chunk, into the history the next one is sized from.
static void record_queue_peaks(DeviceState *D, const QueueSizing &q, double rays_per_sample, double queries_per_sample)
{
    DeviceState::QueueHistory &H = D->qhist;
    if (q.hist_ok) { H.rays_per_sample = std::max(H.rays_per_sample, rays_per_sample); H.queries_per_sample = std::max(H.queries_per_sample, queries_per_sample); }
    else { H.valid = true; H.key = q.key; H.rays_per_sample = rays_per_sample; H.queries_per_sample = queries_per_sample; }
}

// ---- render orchestration ---------------------------------------------------------------------------------
// Samples per pipeline pass.  The kernels are persistent grids that take their work from device-side counters, so a
// bigger chunk means fewer launches, fewer drain phases and longer-lived LDS ray stacks: measured on MI355X (Cornell
// 1080p x 64 spp, two chunks in flight) 4 Mi: 77.4 ms, 8 Mi: 72.3, 32 Mi: 68.9, 64 Mi: 67.7 per frame.  A device-side
// render (rt_render_tiles_device: bench, multi-GPU) therefore takes 64 Mi samples at a time -- 1.1 GB of per-sample
// buffers; the queues are sized from measurement, not from 2^bounce -- while a job (rt_render_begin) keeps 8 Mi chunks:
// its caller watches the image fill band by band, and a band is a chunk.
static size_t chunk_samples_limit(bool job)
{
    const char *e = getenv("RT_CHUNK_SAMPLES");
    long long v = e ? atoll(e) : 0;
    if (v < 4096) v = job ? (8LL << 20) : (64LL << 20);
    return (size_t)v;
}

// Chunks of a frame in flight at once (each on its own stream with its own working set); RT_STREAMS=n in the
// environment (1..RT_STREAMS) overrides the default (tuning / debugging).
static int render_streams(uint64_t n_chunks)
{
    const char *e = getenv("RT_STREAMS");
    // measured on MI355X, round 2.  Many small chunks (Cornell frame in 16 chunks of 8 Mi samples): 1: 74.9 ms, 2: 71.8,
    // 3: 73.5, 4: 71.7 -- a second chunk fills the first one's launch gaps and drain phases, three slots leave the
    // sixteenth chunk alone at the end, two need the least memory.  One or two whole-frame chunks (64 Mi samples): the
    // kernels are persistent grids that fill the GPU on their own and the frame is the sum of them -- a second chunk
    // in flight only makes them share it: 1: 50.5 ms, 2: 51.2.  Round 4, with kernels a third faster: the drain phase of a
    // persistent launch (its last workgroups, its overflow pass) is now worth filling with the other chunk -- Cornell frame
    // 36.15 -> 35.64 ms, the 102 k-triangle frame 21.81 -> 20.66; four chunks of 32 Mi samples stay slower (37.2).
    const int v = e ? atoi(e) : (n_chunks <= 1 ? 1 : 2);
    return v < 1 ? 1 : (v > RT_STREAMS ? RT_STREAMS : v);
}

// ray_factor / query_factor: queue entries per sample to provide (<= 0: the worst case, every hit spawning `fan` rays level
// after level); an overflow is detected on the device and reported, never silent
static rt_status ensure_workspace(DeviceState *D, int slot, size_t samples, int bounce, size_t list_pixels, int fan = 2, bool caustic = false,
                                  double ray_factor = 0, double query_factor = 0, bool reproducible = false)
{
    rt_status st;
    Workspace &w = D->ws[slot];
    if (bounce < 0) bounce = 0;
    if (bounce > 12) return fail(RT_ERR_LIMIT, "bounce limit %d > 12", bounce);
    // worst case: every hit spawns `fan` rays, level after level (overflow is detected and reported)
    double grow = 1.0;
    for (int b = 0; b < bounce; b++) grow *= fan;
    unsigned long long rq_cap = (unsigned long long)std::min(4.0e9, (double)samples * grow);
    unsigned long long pq_cap = (unsigned long long)std::min(4.0e9, (double)samples * grow * 2.0);    // hits on levels 1..bounce
    if (ray_factor > 0) rq_cap = std::min<unsigned long long>(rq_cap, (unsigned long long)((double)samples * ray_factor) + 65536ull);
    if (query_factor > 0) pq_cap = std::min<unsigned long long>(pq_cap, (unsigned long long)((double)samples * query_factor) + 65536ull);
    const unsigned long long lim = 1ull << 28;
    if (rq_cap > lim) rq_cap = lim;
    if (pq_cap > lim) pq_cap = lim;
    if (const char *e = getenv("RT_QUEUE_CAP")) {          // tests only: force a small queue to exercise the overflow report
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v >= 64) { rq_cap = std::min(rq_cap, v); pq_cap = std::min(pq_cap, v); }
    }
    if (rq_cap < 64) rq_cap = 64;
    if (pq_cap < 64) pq_cap = 64;
    if ((st = w.sample_rgb.ensure(samples * 12))) return st;
    if ((st = w.sample_z.ensure(samples * 4))) return st;
    if ((st = w.sample_hit.ensure(samples))) return st;
    if (reproducible && (st = w.sample_fx.ensure(samples * 24))) return st;
    for (int i = 0; i < 2; i++) for (int k = 0; k < 5; k++) if ((st = w.rq[i][k].ensure((size_t)rq_cap * 16))) return st;
    for (int k = 0; k < 3; k++) if ((st = w.pq[k].ensure((size_t)pq_cap * 16))) return st;
    if (caustic) for (int k = 0; k < 3; k++) if ((st = w.cq[k].ensure((size_t)pq_cap * 16))) return st;
    if ((st = w.counts.ensure(CNT_TOTAL * 4))) return st;
    if (D->scene.max_bvh_depth > RT_BVH_LDS && (st = w.bvh_spill.ensure(SPILL_BYTES))) return st;
    if ((st = w.pixel_list.ensure(std::max<size_t>(list_pixels, 1) * 4))) return st;
    if (!D->stats.p) { if ((st = D->stats.ensure(STATS_BYTES))) return st; }
    if (!w.stream) HIP_TRY(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));      // (slot 0 uses its own only in a pipelined frame)
    w.samples = samples; w.rq_cap = (uint32_t)rq_cap; w.pq_cap = (uint32_t)pq_cap;
    return RT_OK;
}

static DevWork make_work(DeviceState *D, int slot)
{
    const Workspace &w = D->ws[slot];
    DevWork W;
    W.sample_rgb = (float *)w.sample_rgb.p; W.sample_z = (float *)w.sample_z.p; W.sample_hit = (uint8_t *)w.sample_hit.p;
    for (int i = 0; i < 2; i++) {
        W.rq[i].a = (float4 *)w.rq[i][0].p; W.rq[i].b = (float4 *)w.rq[i][1].p; W.rq[i].c = (float4 *)w.rq[i][2].p;
        W.rq[i].d = (uint4 *)w.rq[i][3].p; W.rq[i].e = (float4 *)w.rq[i][4].p; W.rq[i].cap = w.rq_cap;
    }
    W.pq.qa = (float4 *)w.pq[0].p; W.pq.qb = (float4 *)w.pq[1].p; W.pq.qc = (float4 *)w.pq[2].p; W.pq.cap = w.pq_cap;
    W.cq.qa = (float4 *)w.cq[0].p; W.cq.qb = (float4 *)w.cq[1].p; W.cq.qc = (float4 *)w.cq[2].p; W.cq.cap = w.cq[0].p ? w.pq_cap : 0;
    W.counts = (uint32_t *)w.counts.p; W.pixel_list = (uint32_t *)w.pixel_list.p;
    W.bvh_spill = D->scene.max_bvh_depth > RT_BVH_LDS ? (uint32_t *)w.bvh_spill.p : nullptr;
    W.stats = (unsigned long long *)D->stats.p;
    return W;
}

// Work queued by an earlier asynchronous render still owns the working sets: order `st` behind it.
rt_status order_after_pending(DeviceState *D, hipStream_t st)
{
    if (D->last_pending && D->last_done) HIP_TRY(hipStreamWaitEvent(st, D->last_done, 0));
    return RT_OK;
}
// The statistics block keeps its counters RT_STAT_STRIDE apart (rt_dev.h): counters [first, first + n) as a dense array, and back to zero
static hipError_t stats_read(const void *dev, int first, int n, unsigned long long *out)
{
    return hipMemcpy2D(out, 8, (const unsigned long long *)dev + ST_AT(first), (size_t)RT_STAT_STRIDE * 8, 8, (size_t)n, hipMemcpyDeviceToHost);
}
static hipError_t stats_zero(void *dev, int first, int n, hipStream_t st)
{
    if (first == 0 && n == ST_COUNT) return hipMemsetAsync(dev, 0, STATS_BYTES, st);
    for (int i = first; i < first + n; i++)
        if (hipError_t e = hipMemsetAsync((unsigned long long *)dev + ST_AT(i), 0, 8, st)) return e;
    return hipSuccess;
}

// The verdict of the asynchronous renders still pending: waits for the last one and reads the drop counter (dropped rays / photon
// queries of the renders since it was last cleared; a host-synchronous read); drops clear the counter and invalidate the queue history (the next render starts from the worst case again).  What the caller does with the
// verdict is its own: a render keeps it in async_overflow for rt_render_check, which reports it.
static rt_status collect_pending_verdict(DeviceState *D, unsigned long long *drops)
{
    *drops = 0;
    if (!D->last_pending || !D->last_done) return RT_OK;
    HIP_TRY(hipEventSynchronize(D->last_done));
    D->last_pending = false;
    if (!D->stats.p) return RT_OK;
    HIP_TRY(stats_read(D->stats.p, ST_QUEUE_OVERFLOW, 1, drops));
    if (*drops) { D->qhist.valid = false; HIP_TRY(hipMemset((unsigned long long *)D->stats.p + ST_AT(ST_QUEUE_OVERFLOW), 0, 8)); }
    return RT_OK;
}

// camera set-up of RenderPixel, FIN/main.cpp:205-224 (tan in double, everything else float)
void camera_setup(const rt_camera &cam, DevCamera &dc)
{
    using rt::Point3;
    const float theta = cam.fov;
    const float l = cam.focaldist;
    const float h = (float)(2 * l * tan(theta / 2 * (M_PI / 180)));
    const float w = h * (float)cam.width / cam.height;
    Point3 b(-w / 2, h / 2, -l);
    const float u = w / cam.width;
    const float v = -h / cam.height;
    const float du = u / 2, dv = v / 2;
    b.x += du; b.y += dv;
    Point3 up(cam.up[0], cam.up[1], cam.up[2]);
    Point3 z_new = Point3(cam.dir[0], cam.dir[1], cam.dir[2]) * (float)-1;
    Point3 x_new = up ^ z_new;
    up.Normalize(); z_new.Normalize(); x_new.Normalize();
    memcpy(dc.pos, cam.pos, 12);
    dc.m[0] = x_new.x; dc.m[1] = x_new.y; dc.m[2] = x_new.z;
    dc.m[3] = up.x; dc.m[4] = up.y; dc.m[5] = up.z;
    dc.m[6] = z_new.x; dc.m[7] = z_new.y; dc.m[8] = z_new.z;
    dc.b[0] = b.x; dc.b[1] = b.y; dc.b[2] = b.z;
    dc.u = u; dc.v = v; dc.dof = cam.dof; dc.width = cam.width; dc.height = cam.height;
}

rt_status validate_render(const rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *t)
{
    if (!cam || !p || !t) return fail(RT_ERR_ARG, "render: camera, params and tile range are required");
    if (cam->width <= 0 || cam->height <= 0 || (long long)cam->width * cam->height > (1LL << 28)) return fail(RT_ERR_ARG, "render: bad image size %dx%d", cam->width, cam->height);
    if ((unsigned long long)cam->width * cam->height * (unsigned long long)p->max_sample >= (1ull << 32))
        return fail(RT_ERR_LIMIT, "render: width*height*max_sample must stay below 2^32 (sample ids are 32-bit)");
    if (p->min_sample < 1 || p->max_sample < p->min_sample || p->max_sample > 4096) return fail(RT_ERR_ARG, "render: need 1 <= min_sample <= max_sample <= 4096");
    if (p->shade_model < RT_SHADE_FIN || p->shade_model > RT_SHADE_P3)
        return fail(RT_ERR_ARG, "render: unknown shade model %d", p->shade_model);
    if (p->shade_model == RT_SHADE_P6 && p->bounce > 7) return fail(RT_ERR_LIMIT, "render: RT_SHADE_P6 supports bounce <= 7");
    if (p->shade_model == RT_SHADE_P12 && (p->hemisphere_sample < 1 || p->hemisphere_sample > 256))
        return fail(RT_ERR_ARG, "render: hemisphere_sample must be 1..256 for RT_SHADE_P12");
    if (p->knn_k < 1 || p->knn_k > 65536 || !(p->knn_radius > 0)) return fail(RT_ERR_ARG, "render: bad photon gather parameters");
    if (!(p->gamma > 0)) return fail(RT_ERR_ARG, "render: gamma must be positive");
    if (p->caustic_k < 0 || p->caustic_k > 65536 || (p->caustic_k > 0 && !(p->caustic_radius > 0))) return fail(RT_ERR_ARG, "render: bad caustic gather parameters");
    if (t->tile_w <= 0 || t->tile_h <= 0 || t->stride <= 0 || t->first < 0) return fail(RT_ERR_ARG, "render: bad tile range");
    if (p->shadow_samples > 32) return fail(RT_ERR_LIMIT, "render: at most 32 shadow samples per light");
    if (p->photon_count < 0 || p->photon_count > (1 << 28) || (p->photon_count > 0 && (p->photon_bounce < 1 || p->photon_bounce > 8)))
        return fail(RT_ERR_ARG, "render: need 0 <= photon_count <= 2^28 and 1 <= photon_bounce <= 8");
    return RT_OK;
}

// The events run_pipeline leaves on a stream when statistics are wanted: cls[i] is what ran between ev[i - 1] and ev[i]
// (TM_START: nothing that is counted -- the pass begins there).
enum TimingClass { TM_START, TM_PRIMARY, TM_BOUNCE, TM_GATHER };
struct Timing { std::vector<Event> ev; std::vector<TimingClass> cls; };

// Levels of the ray tree below the primary rays.  P6: a side ray is spawned when its refraction ray ARRIVES, one queue level
// later than a sibling would be, so a path can take up to two levels per bounce.
static int tree_levels(const rt_params &P) { return P.shade_model == RT_SHADE_P6 ? 2 * P.bounce : P.bounce; }

// One tracing pass over a chunk on its stream: primary samples, the levels of the ray tree, the gathers against the photon maps,
// and (reproducible mode) the fold of the secondary plane -- the chunk's samples are final in W.sample_* behind it.
static rt_status run_pipeline(DeviceState *D, hipStream_t st, const DevWork &W, const rt_params &P, Timing *tm, const RenderPass &pass)
{
    unsigned long long *const fx = pass.fx;
    auto mark = [&](TimingClass cls) -> rt_status {
        if (!tm) return RT_OK;
        Event e;
        HIP_TRY(e.create());
        HIP_TRY(hipEventRecord(e, st));
        tm->ev.push_back(std::move(e)); tm->cls.push_back(cls);
        return RT_OK;
    };
    rt_status s;
    // queue counters for levels 0..15 and the photon queue are reset; the pixel list count survives
    HIP_TRY(hipMemsetAsync(W.counts, 0, CNT_RESET * 4, st));
    // reproducible mode (fx != NULL): the secondary plane of the chunk's slots starts at zero with the chunk's first pass; every
    // pass folds it into sample_rgb at its end and leaves it zero behind (k_fold_fx), which is where a second pass finds it
    const size_t chunk_slots = (size_t)pass.npix * (size_t)pass.max_sample;
    if (fx && pass.mode != 1) HIP_TRY(hipMemsetAsync(fx, 0, chunk_slots * 24, st));
    if ((s = mark(TM_START))) return s;
    rtk_launch_primary(st, D->scene, W, P, pass, RT_TRACE_BLOCKS);
    if ((s = mark(TM_PRIMARY))) return s;
    const int max_level = tree_levels(P);
    // k_wavefront's overflow (level-1 queue) first goes through a second k_wavefront pass; what overflows again, and the
    // models without that kernel, take one launch per level
    int first_level = 1;
    if (max_level >= 2 && rtk_launch_wavefront_queue(st, D->scene, W, P, pass)) first_level = 2;
    // (further passes of the same kernel over what the second one could not keep were measured: 1 / 2 / 3 / 4 queue passes, tracer ms behind
    // the first pass, Cornell 0.34 / 0.36 / 0.40 / 0.44, C3 13.0 / 13.0 / 13.1 / 13.1 -- the second pass takes everything that matters)
    for (int level = first_level; level <= max_level && level < 15; level++)
        rtk_launch_bounce(st, D->scene, W, P, level, RT_TRACE_BLOCKS, fx);
    if ((s = mark(TM_BOUNCE))) return s;
    // one k_gather launch over a queue of the working set against one of the two maps
    auto gather = [&](const DevPhotonMap &pm, const DevPhotonQueue &q, int count_at, int next_at, int k, float radius, const DevBuf &rk2) -> rt_status {
        GatherRequest g = {};
        g.sample_rgb = W.sample_rgb; g.stats = W.stats; g.fx = fx;
        g.pm = pm; g.q = q; g.count = W.counts + count_at; g.k = k; g.radius = radius;
        // reproducible mode: the per-cell hints are off (they pick which of two exact paths, with two summation orders, a query
        // takes, from whichever query of the cell was answered last)
        g.next_batch = W.counts + next_at; g.cell_rk2 = fx ? nullptr : (float *)rk2.p;
        rtk_launch_gather(st, g, gather_blocks());
        return mark(TM_GATHER);
    };
    if ((s = ensure_cell_start(D, false, P.knn_k, P.knn_radius, st))) return s;
    if (D->scene.pm.n_leaves && (s = gather(D->scene.pm, W.pq, CNT_PHOTONQ, CNT_GATHER_NEXT, P.knn_k, P.knn_radius, D->maps[0].cell_rk2))) return s;
    if (D->scene.cm.n_leaves && P.caustic_k > 0 && W.cq.cap) {
        // the P13-family models queued their caustic lookups separately: same kernel on the second map
        if ((s = ensure_cell_start(D, true, P.caustic_k, P.caustic_radius, st))) return s;
        if ((s = gather(D->scene.cm, W.cq, CNT_CAUSTICQ, CNT_GATHER_NEXT2, P.caustic_k, P.caustic_radius, D->maps[1].cell_rk2))) return s;
    }
    // the secondary plane goes into the samples before k_resolve
    if (fx) rtk_launch_fold_fx(st, W.sample_rgb, fx, chunk_slots);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// the counting fields of rt_stats from the statistics block (the timing fields, pixels, attempts and streams are left as they are)
static rt_status read_counters(const void *stats_dev, rt_stats &R)
{
    unsigned long long hs[ST_COUNT];
    HIP_TRY(stats_read(stats_dev, 0, ST_COUNT, hs));
    R.rays_primary = hs[ST_RAYS_PRIMARY]; R.rays_shadow = hs[ST_RAYS_SHADOW]; R.rays_reflect = hs[ST_RAYS_REFLECT];
    R.rays_refract = hs[ST_RAYS_REFRACT]; R.instance_visits = hs[ST_INSTANCE_VISITS]; R.bvh_nodes_visited = hs[ST_BVH_NODES];
    R.tris_tested = hs[ST_TRIS]; R.photon_queries = hs[ST_PHOTON_QUERIES]; R.photons_visited = hs[ST_PHOTONS_VISITED];
    R.samples = hs[ST_RAYS_PRIMARY];
    R.gather_rounds = hs[ST_GATHER_ROUNDS]; R.gather_slow = hs[ST_GATHER_SLOW]; R.gather_leaf_reads = hs[ST_GATHER_LEAF_READS];
    R.peak_rays = hs[ST_PEAK_RAYS]; R.peak_queries = hs[ST_PEAK_QUERIES];
    return RT_OK;
}

// A call's tile walk: walk index q runs tile-major over the call's tiles (tile_px slots per tile, row-major inside a tile);
// the slots of a ragged tile that lie outside the image belong to no pixel.
struct TileWalk {
    const DevTiles &dt; int width, height; uint64_t tile_px;
    void tile_origin(uint64_t k, int &x, int &y) const       // top-left pixel of the walk's k-th tile
    {
        const int t = dt.first + (int)k * dt.stride;
        x = (t % dt.tiles_x) * dt.tile_w; y = (t / dt.tiles_x) * dt.tile_h;
    }
    int64_t offset(uint64_t q) const                            // image offset of slot q, or -1: outside the image
    {
        int x, y;
        tile_origin(q / tile_px, x, y);
        const int w = (int)(q % tile_px);
        x += w % dt.tile_w; y += w / dt.tile_w;
        return x < width && y < height ? (int64_t)y * width + x : -1;
    }
    uint64_t pixels(uint64_t q0, uint64_t q1) const             // image pixels of slots [q0, q1), both on tile boundaries
    {
        uint64_t n = 0;
        for (uint64_t k = q0 / tile_px; k < q1 / tile_px; k++) {
            int x, y;
            tile_origin(k, x, y);
            const int w = std::min(dt.tile_w, width - x), h = std::min(dt.tile_h, height - y);
            if (w > 0 && h > 0) n += (uint64_t)w * h;
        }
        return n;
    }
};

#define RT_ERR_OVERFLOW_RETRY (-1000)     /* internal: queues sized from history overflowed; render again with worst-case queues */

namespace {
// a job's chunk on its way to the caller's planes: slots [q0, q0 + npix) of the tile walk, `done` behind its last kernel
struct InFlight { uint64_t q0; uint32_t npix; Event done; };

// One attempt at a render call: what the phases of render_tiles_once share.  The members below are those phases, in the order
// they run.  Every event and scratch buffer of the attempt goes with it, on whichever path the attempt is left, and the device
// claim after them.
struct RenderAttempt {
    // one host call at a time per (scene, device): the working sets are not shared between concurrent calls
    DeviceClaim claim;
    rt_scene *const s; DeviceState *const D;
    const rt_camera *const cam; const rt_params *const p; const rt_tile_range *const tiles; const RenderRequest &req;
    rt_job *const job;
    const bool sync, want_stats;
    hipStream_t stream = nullptr;       // the caller's, or the device's own
    // the plan (plan_chunks, choose_queue_sizing)
    DevCamera dc; DevTiles dt;
    uint64_t tile_px = 0, total_px = 0, ppc = 0, n_chunks = 0;
    bool pipelined = false, reproducible = false, features = false;
    QueueSizing qs;
    // the slots (acquire_slots, fork_slots)
    int n_slots = 0;
    DevWork Ws[RT_STREAMS];
    unsigned long long *Fx[RT_STREAMS] = {};
    bool tables_touched = false;
    bool resolve_waits[RT_STREAMS] = {};        // the slot's stream is not behind e_fork yet: its first k_resolve waits for it
    // the output targets (setup_outputs)
    ScopedDevBuf job_packed_buf, stage[N_PLANES];
    void *packed_dev = nullptr;
    size_t rec_bytes = 8;               // bytes per packed record: 8, or 24 with the linear plane (the 8-byte record, linear r, g, b, 4 zero bytes)
    bool job_packed = false, linear = false, feat_by_walk = false;
    DevFeatures fdev;
    float *variance_dev = nullptr;      // where k_resolve writes the variance plane (NULL: not asked for)
    // timing and completion events; chunks in flight (job mode), delivered oldest-first for progress and the band copy
    Timing tm[RT_STREAMS];
    Event e_begin, e_end, e_fork;
    std::vector<std::pair<Event, Event>> resolve_ev;
    std::vector<InFlight> flight;
    int attempt_progress = 0;

    RenderAttempt(rt_scene *s_, DeviceState *D_, const rt_camera *cam_, const rt_params *p_, const rt_tile_range *tiles_, const RenderRequest &req_)
        : claim(D_), s(s_), D(D_), cam(cam_), p(p_), tiles(tiles_), req(req_), job(req_.job), sync(req_.sync),
          want_stats(req_.stats_out != nullptr || req_.job != nullptr) {}

    TileWalk walk() const { return TileWalk{dt, cam->width, cam->height, tile_px}; }
    // slot 0 runs on `stream` itself; the other slots' streams start after everything already queued on
    // `stream` (fork) and `stream` waits for them at the end (join), so the call keeps stream-order semantics
    hipStream_t slot_stream(int slot) const { return (slot == 0 && !pipelined) ? stream : D->ws[slot].stream; }

    // The device is prepared and claimed (the constructor): order the call behind the render in flight and collect its verdict.
    rt_status enter()
    {
        if (!claim.ok) return fail(RT_ERR_STATE, "render: another call on this scene is using device %d", D->device);
        rt_status st;
        stream = req.stream ? req.stream : D->stream;
        if ((st = order_after_pending(D, stream))) return st;
        if (!D->last_done) HIP_TRY(hipEventCreateWithFlags(&D->last_done, hipEventDisableTiming));
        if (D->last_pending && (sync || want_stats)) {
            // this call will clear and read the shared drop counter: the verdict of the asynchronous renders before it is
            // collected first and kept for rt_render_check ("queue overflow is always reported")
            unsigned long long drops = 0;
            if ((st = collect_pending_verdict(D, &drops))) return st;
            if (drops) D->async_overflow = true;
        }
        return RT_OK;
    }

    // The tile walk of the call, cut into chunks of ppc pixels, and how many of them are in flight at once.
    void plan_chunks()
    {
        camera_setup(*cam, dc);
        dt.tile_w = tiles->tile_w; dt.tile_h = tiles->tile_h; dt.first = tiles->first; dt.stride = tiles->stride;
        dt.tiles_x = (cam->width + dt.tile_w - 1) / dt.tile_w;
        const int tiles_y = (cam->height + dt.tile_h - 1) / dt.tile_h;
        dt.tiles_total = dt.tiles_x * tiles_y;
        dt.n_tiles = dt.first >= dt.tiles_total ? 0 : (dt.tiles_total - dt.first + dt.stride - 1) / dt.stride;
        tile_px = (uint64_t)dt.tile_w * dt.tile_h;
        total_px = tile_px * (uint64_t)dt.n_tiles;

        const size_t limit = chunk_samples_limit(job != nullptr);
        ppc = std::max<uint64_t>(1, limit / (uint64_t)p->max_sample);
        ppc = std::max<uint64_t>(tile_px, ppc / tile_px * tile_px);
        ppc = std::min<uint64_t>(ppc, std::max<uint64_t>(total_px, 1));
        n_chunks = total_px ? (total_px + ppc - 1) / ppc : 0;
        // FRAME PIPELINING (opt-in: RT_FRAME_PIPELINE=1).  An asynchronous render behind another one that is still in flight runs all of its
        // slots on the library's own streams and lets its tracing and gathering start at once: they touch nothing but the slot's working
        // set, which the slot's stream already orders, and read scene tables no stream-ordered work of the caller can change.  Only
        // k_resolve, which writes the caller's buffers, waits for what the caller's stream holds before this call (e_fork) -- the frame
        // before it, an all-gather of its tiles, a copy of the image; frames of one chunk alternate between two slots.  What it is for:
        // the tile exchange of a multi-GPU step sits between two frames, and this puts the next frame's rays beside it.  Why it is not the
        // default: measured on ONE GPU (r4, profiles/r04_experiments.json) it gains nothing where there is no exchange to hide -- a rank's
        // share at N = 2 / 4 / 8: 18.73 / 10.14 / 5.39 ms against 18.73 / 10.14 / 5.33 -- and costs the two-chunk frames their lockstep
        // (both chunks tracing, then both gathering: Cornell 36.4 against 36.0 ms, 102 k triangles 21.75 against 20.64: a tracer and a gather
        // side by side take each other's LDS); with an exchange beside persistent grids that leave no LDS free it is unmeasured.
        const char *e = getenv("RT_FRAME_PIPELINE");
        pipelined = e && atoi(e) != 0 && !sync && !want_stats && D->last_pending && total_px > 0;
        const int streams_wanted = render_streams(pipelined ? std::max<uint64_t>(n_chunks, 2) : n_chunks);
        if (streams_wanted < 2) pipelined = false;              // RT_STREAMS=1: one chunk at a time, as asked
        n_slots = pipelined ? streams_wanted : (int)std::min<uint64_t>(std::max<uint64_t>(n_chunks, 1), (uint64_t)streams_wanted);
        // the render's mode is the scene's flags as they are now: kernels enqueued by this call keep it whatever is set later
        reproducible = (s->render_flags.load() & RT_RENDER_REPRODUCIBLE) != 0;
        // first-hit feature planes (k_features after each chunk's last resolve): only when a plane was asked for
        features = (job ? job->host : req.packed ? req.walk : req.dev).features().any();
    }

    // A working set per slot; the attempt goes on with as many as it got.
    rt_status acquire_slots()
    {
        rt_status st;
        const size_t samples = (size_t)ppc * p->max_sample;
        int n_ready = 0;
        for (int i = 0; i < n_slots; i++) {
            if (i > 0 && D->ws[i].samples < samples) {
                // an extra working set is an optimisation: take it only while a comfortable share of the HBM stays
                // free (other ranks rehearsing on the same device, the caller's own tensors)
                size_t free_b = 0, total_b = 0;
                if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); break; }
                const size_t first = D->ws[0].sample_rgb.bytes + D->ws[0].sample_z.bytes + D->ws[0].sample_hit.bytes + 10 * D->ws[0].rq[0][0].bytes +
                                     3 * D->ws[0].pq[0].bytes;
                if (free_b < first + first / 4 + (total_b >> 3)) break;
            }
            if ((st = ensure_workspace(D, i, samples, p->bounce, (size_t)ppc, qs.key.fan, qs.key.caustic, qs.ray_factor, qs.query_factor,
                                       reproducible))) return st;
            Ws[i] = make_work(D, i);
            if (reproducible) Fx[i] = (unsigned long long *)D->ws[i].sample_fx.p;
            if (features && (st = D->ws[i].feat_second.ensure(std::max<uint64_t>(ppc, 1)))) return st;
            n_ready++;
        }
        n_slots = n_ready;
        return RT_OK;
    }

    // Where k_resolve and k_features write.
    rt_status setup_outputs()
    {
        rt_status st;
        // a job that owns only some of the tiles renders into packed records of its own (see scatter_packed)
        job_packed = job != nullptr && tiles->stride != 1;
        rec_bytes = req.rec_bytes;
        packed_dev = req.packed;
        if (job_packed) {
            if ((st = job_packed_buf.ensure(std::max<uint64_t>(total_px, 1) * rec_bytes))) return st;
            packed_dev = job_packed_buf.p;
        }
        linear = packed_dev ? rec_bytes == 24 : req.dev.p[PL_LINEAR] != nullptr;
        // where k_features writes: the caller's image-sized device planes, or -- a strided job, whose rows are shared with other jobs --
        // staging planes indexed by this call's tile walk, scattered on the host like the packed records (scatter_packed)
        // the variance plane goes the same two ways (k_resolve indexes it by the walk when it writes packed records)
        fdev = req.dev.features();
        variance_dev = req.dev.at<float>(PL_VARIANCE);
        feat_by_walk = features && job_packed;
        if (job_packed) {
            Planes staged;
            for (int i = PL_NORMAL; i < N_PLANES; i++) {
                if (!job->host.p[i]) continue;
                if ((st = stage[i].ensure(std::max<uint64_t>(total_px, 1) * PLANE_BYTES[i]))) return st;
                staged.p[i] = stage[i].p;
            }
            if (feat_by_walk) fdev = staged.features();
            variance_dev = staged.at<float>(PL_VARIANCE);
        } else if (packed_dev) {
            // packed planes: the same two pointers, re-aimed into the sections of the caller's buffer
            fdev = req.walk.features();
            feat_by_walk = features;
            variance_dev = req.walk.at<float>(PL_VARIANCE);
        }
        return RT_OK;
    }

    // What goes onto `stream` before the slots fork from it: the statistics' start (or the partial counter reset) and the gathers'
    // start tables.
    rt_status begin_on_stream()
    {
        rt_status st;
        // packed planes: k_resolve writes (zeros included) the records of the call's own tiles, k_features and the variance only
        // the slots of image pixels; everything else of the contribution -- the records of a short rank's missing tile, every
        // section, the rounding -- starts from zero on every call
        const uint64_t written = total_px * rec_bytes;
        if (req.packed_bytes > written)
            HIP_TRY(hipMemsetAsync((uint8_t *)req.packed + written, 0, req.packed_bytes - written, stream));
        if (want_stats) {
            HIP_TRY(stats_zero(Ws[0].stats, 0, ST_COUNT, stream));
            HIP_TRY(e_begin.create()); HIP_TRY(e_end.create());
            HIP_TRY(hipEventRecord(e_begin, stream));
        } else if (!D->last_pending) {
            // the drop counter is read back after every synchronous render (finish) and by rt_render_check after
            // asynchronous ones; consecutive asynchronous renders accumulate into it until it is checked
            HIP_TRY(stats_zero(Ws[0].stats, ST_QUEUE_OVERFLOW, 1, stream));
            HIP_TRY(stats_zero(Ws[0].stats, ST_PEAK_RAYS, 2, stream));
        }
        if ((st = ensure_cell_start(D, false, p->knn_k, p->knn_radius, stream, &tables_touched))) return st;
        if (qs.key.caustic && (st = ensure_cell_start(D, true, p->caustic_k, p->caustic_radius, stream, &tables_touched))) return st;
        return RT_OK;
    }

    // The slots' own streams go behind what `stream` holds now (e_fork), at once or -- a pipelined frame -- at their first k_resolve.
    rt_status fork_slots()
    {
        if (n_slots <= 1 && !pipelined) return RT_OK;
        HIP_TRY(e_fork.create(hipEventDisableTiming));
        HIP_TRY(hipEventRecord(e_fork, stream));
        for (int i = pipelined ? 0 : 1; i < n_slots; i++) {     // (not pipelined: slot 0 IS `stream`)
            // pipelined: the gathers' tables were just rewritten on `stream`, or the frame before used the slots on other streams
            // (slot 0 on the caller's): start behind everything; otherwise only this slot's k_resolve launches wait
            if (!pipelined || tables_touched || !D->last_pipelined) HIP_TRY(hipStreamWaitEvent(slot_stream(i), e_fork, 0));
            else resolve_waits[i] = true;
        }
        return RT_OK;
    }

    // One k_resolve phase over a chunk, between two events when the call wants statistics.
    rt_status resolve(hipStream_t cs, const DevWork &W, ResolveArgs &ra, int phase)
    {
        Event r0, r1;
        if (want_stats) { HIP_TRY(r0.create()); HIP_TRY(r1.create()); HIP_TRY(hipEventRecord(r0, cs)); }
        ra.phase = phase;
        rtk_launch_resolve(cs, W, ra, 2048, linear);
        if (want_stats) { HIP_TRY(hipEventRecord(r1, cs)); resolve_ev.emplace_back(std::move(r0), std::move(r1)); }
        return RT_OK;
    }

    // The chunk that starts at slot q0 of the tile walk, on its slot's stream: the first sample batch and its resolve, the second
    // batch for the pixels that one listed (adaptive renders), the features; a job's chunk is then queued for delivery.
    rt_status render_chunk(uint64_t q0, uint64_t chunk_index)
    {
        rt_status st;
        const int slot = (int)((chunk_index + (pipelined ? D->frame_seq : 0)) % (uint64_t)n_slots);
        const hipStream_t cs = slot_stream(slot);
        const DevWork &W = Ws[slot];
        Timing *tmp = want_stats ? &tm[slot] : nullptr;
        const uint32_t npix = (uint32_t)std::min<uint64_t>(ppc, total_px - q0);
        HIP_TRY(hipMemsetAsync(W.counts + CNT_PIXLIST, 0, 4, cs));
        RenderPass pass = {};
        pass.cam = dc; pass.tiles = dt; pass.q0 = (uint32_t)q0; pass.npix = npix; pass.max_sample = p->max_sample; pass.fx = Fx[slot];
        pass.mode = 0; pass.j0 = 0; pass.ns = p->min_sample;
        if ((st = run_pipeline(D, cs, W, *p, tmp, pass))) return st;
        ResolveArgs ra = {};
        ra.cam = dc; ra.tiles = dt; ra.q0 = pass.q0; ra.npix = npix; ra.min_sample = p->min_sample; ra.max_sample = p->max_sample;
        ra.threshold = p->threshold; memcpy(ra.bg, D->scene.bg, sizeof ra.bg); ra.S = D->scene;
        ra.inv_gamma = (float)(1.0 / p->gamma);                 // powf(x, 1.0/gamma): double quotient narrowed to float
        ra.rgb8 = req.dev.at<uint8_t>(PL_RGB8); ra.z = req.dev.at<float>(PL_Z); ra.count = req.dev.at<uint8_t>(PL_COUNT);
        ra.packed = (uint2 *)packed_dev; ra.rgb_linear = req.dev.at<float>(PL_LINEAR); ra.variance = variance_dev;
        if (resolve_waits[slot]) { HIP_TRY(hipStreamWaitEvent(cs, e_fork, 0)); resolve_waits[slot] = false; }
        if ((st = resolve(cs, W, ra, 0))) return st;
        if (p->max_sample > p->min_sample) {
            pass.mode = 1; pass.j0 = p->min_sample; pass.ns = p->max_sample - p->min_sample;
            if ((st = run_pipeline(D, cs, W, *p, tmp, pass))) return st;
            if ((st = resolve(cs, W, ra, 1))) return st;
        }
        // the feature planes of the chunk, from its finished working set (hit flags, pixel list) on the same stream
        if (features)
            rtk_launch_features(cs, D->scene, W, *p, pass, (uint8_t *)D->ws[slot].feat_second.p, fdev, feat_by_walk);
        HIP_TRY(hipGetLastError());
        if (job) {
            InFlight f; f.q0 = q0; f.npix = npix;
            HIP_TRY(f.done.create(hipEventDisableTiming));
            HIP_TRY(hipEventRecord(f.done, cs));
            flight.push_back(std::move(f));
            while ((int)flight.size() >= n_slots) if ((st = deliver_oldest())) return st;
        }
        return RT_OK;
    }

    // A strided tile range (one job per device on the same caller-owned image): rows are shared with other jobs' tiles,
    // so only this job's pixels may be written -- the chunk's packed 8-byte (24-byte: linear) records come back in one
    // copy and are scattered on the host through the tile walk, and so is the chunk's run of each staged plane (features, variance).
    rt_status scatter_packed(const InFlight &f)
    {
        const TileWalk w = walk();
        const size_t words = rec_bytes / 8;
        std::vector<uint2> rec((size_t)f.npix * words);
        HIP_TRY(hipMemcpy(rec.data(), (const uint2 *)packed_dev + f.q0 * words, (size_t)f.npix * rec_bytes, hipMemcpyDeviceToHost));
        const Planes &h = job->host;
        for (uint32_t i = 0; i < f.npix; i++) {
            const int64_t o = w.offset(f.q0 + i);
            if (o < 0) continue;
            const uint2 v = rec[i * words];
            uint8_t *rgb = h.at<uint8_t>(PL_RGB8) + 3 * o;
            rgb[0] = (uint8_t)(v.x & 255u); rgb[1] = (uint8_t)((v.x >> 8) & 255u); rgb[2] = (uint8_t)((v.x >> 16) & 255u);
            const uint32_t zb = (v.x >> 24) | (v.y << 8);
            memcpy(h.at<float>(PL_Z) + o, &zb, 4);
            h.at<uint8_t>(PL_COUNT)[o] = (uint8_t)(v.y >> 24);
            if (words == 3) memcpy(h.at<float>(PL_LINEAR) + 3 * o, &rec[i * words + 1], 12);
        }
        for (int k = PL_NORMAL; k < N_PLANES; k++) {
            if (!stage[k].p) continue;
            const size_t b = PLANE_BYTES[k];
            std::vector<uint8_t> run((size_t)f.npix * b);
            HIP_TRY(hipMemcpy(run.data(), (const uint8_t *)stage[k].p + f.q0 * b, run.size(), hipMemcpyDeviceToHost));
            for (uint32_t i = 0; i < f.npix; i++) {
                const int64_t o = w.offset(f.q0 + i);
                if (o >= 0) memcpy(h.at<uint8_t>(k) + o * b, run.data() + i * b, b);
            }
        }
        return RT_OK;
    }

    // The rows spanned by the chunk's tiles, per plane (tile-major order: a contiguous band of tile rows; a row shared
    // with a chunk still in flight may arrive torn and is copied again when that chunk finishes).
    rt_status copy_band(const InFlight &f)
    {
        const TileWalk w = walk();
        int x, y0, y1;
        w.tile_origin(f.q0 / tile_px, x, y0);
        w.tile_origin((f.q0 + f.npix - 1) / tile_px, x, y1);
        y1 = std::min(cam->height, y1 + dt.tile_h);
        const size_t o = (size_t)y0 * cam->width, n = y1 > y0 ? (size_t)(y1 - y0) * cam->width : 0;
        for (int k = 0; k < N_PLANES && n; k++)
            if (req.dev.p[k])
                HIP_TRY(hipMemcpy(job->host.at<uint8_t>(k) + o * PLANE_BYTES[k], req.dev.at<uint8_t>(k) + o * PLANE_BYTES[k],
                                  n * PLANE_BYTES[k], hipMemcpyDeviceToHost));
        return RT_OK;
    }

    // Job mode: the oldest chunk in flight, once the GPU is done with it, into the caller's host planes, and the job's progress.
    rt_status deliver_oldest()
    {
        const InFlight f = std::move(flight.front());
        flight.erase(flight.begin());
        HIP_TRY(hipEventSynchronize(f.done));
        if (rt_status st = job_packed ? scatter_packed(f) : copy_band(f)) return st;
        // monotone also when the frame is rendered a second time with larger queues (RT_ERR_OVERFLOW_RETRY)
        attempt_progress += (int)walk().pixels(f.q0, f.q0 + f.npix);
        int seen = job->progress.load();
        while (attempt_progress > seen && !job->progress.compare_exchange_weak(seen, attempt_progress)) {}
        return RT_OK;
    }

    // The chunks still in flight are delivered (also after a stop), and `stream` is put behind every slot's stream.
    rt_status drain_and_join()
    {
        while (job && !flight.empty()) if (rt_status st = deliver_oldest()) return st;
        if (n_slots <= 1 && !pipelined) return RT_OK;
        for (int i = pipelined ? 0 : 1; i < n_slots; i++) {
            Event e_join;
            HIP_TRY(e_join.create(hipEventDisableTiming));
            HIP_TRY(hipEventRecord(e_join, slot_stream(i)));
            HIP_TRY(hipStreamWaitEvent(stream, e_join, 0));
        }
        return RT_OK;
    }

    // A synchronising call waits for the frame, reads its verdict and records its queue peaks; an asynchronous one leaves
    // `last_done` behind it for the next call and rt_render_check.
    rt_status finish()
    {
        if (want_stats) HIP_TRY(hipEventRecord(e_end, stream));
        if (!sync && !want_stats) {
            HIP_TRY(hipEventRecord(D->last_done, stream));
            D->last_pending = true;
            D->last_pipelined = pipelined;
            if (pipelined) D->frame_seq += n_chunks;
            return RT_OK;
        }
        HIP_TRY(hipStreamSynchronize(stream));
        D->last_pending = false;
        D->last_pipelined = false;
        // a dropped ray or photon query means a wrong image: never RT_OK, whether or not statistics were asked for
        unsigned long long tail[ST_COUNT - ST_QUEUE_OVERFLOW];
        HIP_TRY(stats_read(D->stats.p, ST_QUEUE_OVERFLOW, ST_COUNT - ST_QUEUE_OVERFLOW, tail));
        const unsigned long long drops = tail[0], peak_r = tail[ST_PEAK_RAYS - ST_QUEUE_OVERFLOW], peak_q = tail[ST_PEAK_QUERIES - ST_QUEUE_OVERFLOW];
        if (drops) {
            D->qhist.valid = false;
            if (D->qhist_used && !(job && job->stop.load())) return RT_ERR_OVERFLOW_RETRY;      // sized from history: once more, worst case
            return fail(RT_ERR_LIMIT, "render: a ray/photon queue overflowed (%llu drops); lower RT_CHUNK_SAMPLES or the bounce limit", drops);
        }
        const double per = (double)std::max<uint64_t>(1, ppc * (uint64_t)p->max_sample);
        record_queue_peaks(D, qs, (double)peak_r / per, (double)peak_q / per);
        return RT_OK;
    }

    rt_status assemble_stats()
    {
        if (!want_stats) return RT_OK;
        rt_stats R;
        memset(&R, 0, sizeof R);
        if (rt_status st = read_counters(Ws[0].stats, R)) return st;
        // per-stream intervals between consecutive marks: with two chunks in flight a kernel shares the GPU
        // with the other stream's kernels, so these are durations under overlap (the same thing rocprofv3 reports)
        for (int sl = 0; sl < n_slots; sl++)
            for (size_t i = 1; i < tm[sl].ev.size(); i++) {
                if (tm[sl].cls[i] == TM_START) continue;
                float ms = 0;
                HIP_TRY(hipEventElapsedTime(&ms, tm[sl].ev[i - 1], tm[sl].ev[i]));
                if (tm[sl].cls[i] == TM_PRIMARY) { R.ms_primary += ms; R.launches_primary++; }
                else if (tm[sl].cls[i] == TM_BOUNCE) { R.ms_bounce += ms; R.launches_bounce += (uint64_t)std::max(0, std::min(tree_levels(*p), 14)); }
                else { R.ms_gather += ms; R.launches_gather++; }
            }
        R.ms_trace = R.ms_primary + R.ms_bounce;
        R.launches_trace = R.launches_primary + R.launches_bounce;
        R.streams = (uint64_t)n_slots;
        for (auto &pr : resolve_ev) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, pr.first, pr.second));
            R.ms_resolve += ms; R.launches_resolve++;
        }
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, e_begin, e_end));
        R.ms_total = ms;
        R.pixels = walk().pixels(0, total_px);
        if (req.stats_out) *req.stats_out = R;
        if (job) job->stats = R;
        return RT_OK;
    }
};
}   // namespace

static rt_status render_tiles_once(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles, int device,
                                   const RenderRequest &req, bool worst_case)
{
    rt_status st = validate_render(s, cam, p, tiles);
    if (st) return st;
    DeviceState *D = nullptr;
    if ((st = prepare_device(s, device, &D))) return st;
    RenderAttempt A(s, D, cam, p, tiles, req);
    if ((st = A.enter())) return st;
    A.plan_chunks();
    A.qs = choose_queue_sizing(D, *p, worst_case, req.sync || req.job != nullptr);      // (sets D->qhist_used: before anything is launched)
    if ((st = A.acquire_slots())) return st;
    if ((st = A.setup_outputs())) return st;
    if ((st = A.begin_on_stream())) return st;
    if ((st = A.fork_slots())) return st;
    uint64_t chunk_index = 0;
    for (uint64_t q0 = 0; q0 < A.total_px; q0 += A.ppc, chunk_index++) {
        if (req.job && req.job->stop.load()) break;
        if ((st = A.render_chunk(q0, chunk_index))) return st;
    }
    if ((st = A.drain_and_join())) return st;
    if ((st = A.finish())) return st;
    return A.assemble_stats();
}

rt_status render_tiles(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles, int device, const RenderRequest &req)
{
    rt_status st = render_tiles_once(s, cam, p, tiles, device, req, false);
    int attempts = 1;
    if (st == RT_ERR_OVERFLOW_RETRY) {
        attempts = 2;
        st = render_tiles_once(s, cam, p, tiles, device, req, true);
    }
    if (st == RT_OK && req.stats_out) req.stats_out->attempts = (uint64_t)attempts;
    if (st == RT_OK && req.job) req.job->stats.attempts = (uint64_t)attempts;
    return st;
}

// the request of a device-side entry point: the caller's stream, whether the call waits for the frame, where its statistics go
static RenderRequest device_request(void *hip_stream, int sync, rt_stats *stats_out)
{
    RenderRequest req;
    req.stream = (hipStream_t)hip_stream; req.sync = sync != 0; req.stats_out = stats_out;
    return req;
}

// every entry point with image planes (here, rt_exchange.cpp, rt_jobs.cpp): the caller's sizeof first, then the three required planes
rt_status check_outputs(const char *name, const rt_outputs *o)
{
    if (!o) return fail(RT_ERR_ARG, "%s: the plane descriptor is NULL", name);
    if (o->struct_size != (uint32_t)sizeof(rt_outputs))
        return fail(RT_ERR_ARG, "%s: rt_outputs.struct_size is %u, this library's is %zu", name, o->struct_size, sizeof(rt_outputs));
    if (!o->rgb8 || !o->z || !o->count) return fail(RT_ERR_ARG, "%s: rgb8, z and count are required", name);
    return RT_OK;
}

// RenderPixel's outputs (FIN/main.cpp:273-338) into the caller's device planes, with the optional ones of rt_outputs: the linear
// colour and the first hit's normal, albedo, coverage and node (k_features)
static rt_status render_device(const char *name, rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles,
                               int device, void *hip_stream, const rt_outputs *device_planes, int sync, rt_stats *stats_out,
                               float *variance_dev = nullptr)
{
    if (!s) return fail(RT_ERR_ARG, "%s: scene is NULL", name);
    rt_status st = check_outputs(name, device_planes);
    if (st) return st;
    RenderRequest req = device_request(hip_stream, sync, stats_out);
    req.dev = Planes(*device_planes, variance_dev);
    return render_tiles(s, cam, p, tiles, device, req);
}

extern "C" rt_status rt_render_tiles_device(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles,
                                            int device, void *hip_stream, uint8_t *rgb8_dev, float *z_dev, uint8_t *count_dev,
                                            int sync, rt_stats *stats_out)
{
    const rt_outputs o = outputs_of(rgb8_dev, z_dev, count_dev);
    return render_device("rt_render_tiles_device", s, cam, p, tiles, device, hip_stream, &o, sync, stats_out);
}

extern "C" rt_status rt_render_tiles_linear_device(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles,
                                                   int device, void *hip_stream, uint8_t *rgb8_dev, float *z_dev, uint8_t *count_dev,
                                                   float *rgb_linear_dev, int sync, rt_stats *stats_out)
{
    if (!rgb_linear_dev) return fail(RT_ERR_ARG, "rt_render_tiles_linear_device: the linear plane is required");
    const rt_outputs o = outputs_of(rgb8_dev, z_dev, count_dev, rgb_linear_dev);
    return render_device("rt_render_tiles_linear_device", s, cam, p, tiles, device, hip_stream, &o, sync, stats_out);
}

extern "C" rt_status rt_render_tiles_outputs_device(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles,
                                                    int device, void *hip_stream, const rt_outputs *device_planes, int sync, rt_stats *stats_out)
{
    return render_device("rt_render_tiles_outputs_device", s, cam, p, tiles, device, hip_stream, device_planes, sync, stats_out);
}

extern "C" rt_status rt_render_tiles_outputs_var_device(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles,
                                                        int device, void *hip_stream, const rt_outputs *device_planes, float *variance_dev,
                                                        int sync, rt_stats *stats_out)
{
    if (!variance_dev) return fail(RT_ERR_ARG, "rt_render_tiles_outputs_var_device: the variance plane is required");
    return render_device("rt_render_tiles_outputs_var_device", s, cam, p, tiles, device, hip_stream, device_planes, sync, stats_out, variance_dev);
}

extern "C" rt_status rt_render_check(rt_scene *s, int device)
{
    if (!s) return fail(RT_ERR_ARG, "rt_render_check: scene is NULL");
    DeviceState *const D = find_device_state(s, device);
    if (!D) return RT_OK;                                    // nothing was ever rendered there
    HIP_TRY(hipSetDevice(device));
    DeviceClaim claim(D);
    if (!claim.ok) return fail(RT_ERR_STATE, "rt_render_check: another call on this scene is using device %d", device);
    unsigned long long drops = 0;
    if (rt_status st = collect_pending_verdict(D, &drops)) return st;
    const bool earlier = D->async_overflow;
    D->async_overflow = false;
    if (drops || earlier) {
        D->qhist.valid = false;                             // the next render starts from the worst case again
        return fail(RT_ERR_LIMIT, "rt_render_check: a ray/photon queue overflowed (%llu drops) in an asynchronous render", drops);
    }
    return RT_OK;
}

extern "C" rt_status rt_render_counters(rt_scene *s, int device, int reset, rt_stats *out)
{
    if (!s || !out) return fail(RT_ERR_ARG, "rt_render_counters: NULL argument");
    memset(out, 0, sizeof *out);
    DeviceState *const D = find_device_state(s, device);
    if (!D || !D->stats.p) return RT_OK;                     // nothing was ever rendered there
    HIP_TRY(hipSetDevice(device));
    DeviceClaim claim(D);
    if (!claim.ok) return fail(RT_ERR_STATE, "rt_render_counters: another call on this scene is using device %d", device);
    // (the verdict of the asynchronous renders stays with rt_render_check: last_pending is left as it is)
    if (D->last_pending && D->last_done) HIP_TRY(hipEventSynchronize(D->last_done));
    rt_status st = read_counters(D->stats.p, *out);
    if (st) return st;
    if (reset) {
        // the drop counter and the queue peaks belong to the overflow verdict and the queue sizing: not touched
        static_assert(ST_QUEUE_OVERFLOW == ST_PHOTONS_VISITED + 1 && ST_GATHER_ROUNDS == ST_QUEUE_OVERFLOW + 1 && ST_PEAK_RAYS == ST_GATHER_LEAF_READS + 1, "counter layout");
        HIP_TRY(hipMemset(D->stats.p, 0, ST_AT(ST_QUEUE_OVERFLOW) * 8));
        HIP_TRY(hipMemset((unsigned long long *)D->stats.p + ST_AT(ST_GATHER_ROUNDS), 0, ST_AT(ST_PEAK_RAYS - ST_GATHER_ROUNDS) * 8));
    }
    return RT_OK;
}

// ---- single-stage entry points --------------------------------------------------------------------------
extern "C" rt_status rt_trace_rays(rt_scene *s, int shade_model, int device, const float *rays, int64_t n, uint8_t *hit, float *z,
                                   float *p, float *N, int32_t *node, uint8_t *front)
{
    if (!s || n < 0) return fail(RT_ERR_ARG, "rt_trace_rays: NULL scene or negative count");
    if (n > 0 && (!rays || !hit || !z || !p || !N || !node || !front)) return fail(RT_ERR_ARG, "rt_trace_rays: NULL argument");
    if (shade_model < RT_SHADE_FIN || shade_model > RT_SHADE_P3) return fail(RT_ERR_ARG, "rt_trace_rays: unknown shade model");
    DeviceState *D = nullptr;
    rt_status st = prepare_device(s, device, &D);
    if (st) return st;
    if (n == 0) return RT_OK;
    DeviceClaim claim(D);
    if (!claim.ok) return fail(RT_ERR_STATE, "rt_trace_rays: another call on this scene is using device %d", device);
    if ((st = order_after_pending(D, D->stream))) return st;
    const size_t sizes[6] = {(size_t)n, (size_t)n * 4, (size_t)n * 12, (size_t)n * 12, (size_t)n * 4, (size_t)n};
    if ((st = D->t_in.upload(rays, (size_t)n * 24))) return st;
    for (int k = 0; k < 6; k++) if ((st = D->t_out[k].ensure(sizes[k]))) return st;
    TraceOut o = {};
    o.hit = (uint8_t *)D->t_out[0].p; o.z = (float *)D->t_out[1].p; o.p = (float *)D->t_out[2].p; o.N = (float *)D->t_out[3].p;
    o.node = (int32_t *)D->t_out[4].p; o.front = (uint8_t *)D->t_out[5].p;
    rtk_launch_trace(D->stream, D->scene, shade_model, (const float *)D->t_in.p, n, o);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(D->stream));
    void *dst[6] = {hit, z, p, N, node, front};
    for (int k = 0; k < 6; k++) HIP_TRY(hipMemcpy(dst[k], D->t_out[k].p, sizes[k], hipMemcpyDeviceToHost));
    return RT_OK;
}

extern "C" rt_status rt_estimate_irradiance(rt_scene *s, int device, int32_t k, float radius, const float *pos, const float *normal,
                                            int64_t n, float *irr, float *dir)
{
    if (!s || n < 0) return fail(RT_ERR_ARG, "rt_estimate_irradiance: NULL scene or negative count");
    if (n > 0 && (!pos || !normal || !irr || !dir)) return fail(RT_ERR_ARG, "rt_estimate_irradiance: NULL argument");
    if (k < 1 || k > 65536 || !(radius > 0)) return fail(RT_ERR_ARG, "rt_estimate_irradiance: bad k/radius");
    DeviceState *D = nullptr;
    rt_status st = prepare_device(s, device, &D);
    if (st) return st;
    if (n == 0) return RT_OK;
    if (n > (1LL << 28)) return fail(RT_ERR_LIMIT, "rt_estimate_irradiance: too many queries");
    DeviceClaim claim(D);
    if (!claim.ok) return fail(RT_ERR_STATE, "rt_estimate_irradiance: another call on this scene is using device %d", device);
    if ((st = order_after_pending(D, D->stream))) return st;
    if (!D->scene.pm.n_leaves) { memset(irr, 0, (size_t)n * 12); memset(dir, 0, (size_t)n * 12); return RT_OK; }
    std::vector<float4> qa((size_t)n), qb((size_t)n), qc((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        qa[i] = make_float4(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], normal[3 * i]);
        qb[i] = make_float4(normal[3 * i + 1], normal[3 * i + 2], 0, 0);
        qc[i] = make_float4(0, 0, 0, 0);
    }
    std::vector<uint32_t> cnt(1 + (size_t)RT_GATHER_CTRS * RT_CTR_STRIDE, 0u);  // query count, then the work counters as k_gather lays them out
    cnt[0] = (uint32_t)n;
    if ((st = D->t_out[0].upload(qa.data(), (size_t)n * 16))) return st;
    if ((st = D->t_out[1].upload(qb.data(), (size_t)n * 16))) return st;
    if ((st = D->t_out[2].upload(qc.data(), (size_t)n * 16))) return st;
    if ((st = D->t_out[3].ensure((size_t)n * 12))) return st;
    if ((st = D->t_out[4].ensure((size_t)n * 12))) return st;
    if ((st = D->t_in.upload(cnt.data(), cnt.size() * 4))) return st;
    if ((st = ensure_cell_start(D, false, k, radius, D->stream))) return st;
    GatherRequest g = {};
    g.pm = D->scene.pm; g.k = k; g.radius = radius;
    g.q.qa = (float4 *)D->t_out[0].p; g.q.qb = (float4 *)D->t_out[1].p; g.q.qc = (float4 *)D->t_out[2].p; g.q.cap = cnt[0];
    g.count = (const uint32_t *)D->t_in.p; g.next_batch = (uint32_t *)D->t_in.p + 1;
    g.out_irr = (float *)D->t_out[3].p; g.out_dir = (float *)D->t_out[4].p;
    rtk_launch_gather(D->stream, g, gather_blocks());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(D->stream));
    HIP_TRY(hipMemcpy(irr, D->t_out[3].p, (size_t)n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dir, D->t_out[4].p, (size_t)n * 12, hipMemcpyDeviceToHost));
    return RT_OK;
}

extern "C" rt_status rt_shade_rays(rt_scene *s, const rt_params *p, int device, const float *rays, int64_t n, uint8_t *hit, float *rgb, float *z)
{
    if (!s || !p || n < 0) return fail(RT_ERR_ARG, "rt_shade_rays: NULL scene/params or negative count");
    if (n > 0 && (!rays || !hit || !rgb || !z)) return fail(RT_ERR_ARG, "rt_shade_rays: NULL argument");
    rt_camera cam;
    memset(&cam, 0, sizeof cam);
    cam.width = 1; cam.height = 1; cam.fov = 40; cam.focaldist = 1; cam.dir[2] = -1; cam.up[1] = 1;
    rt_tile_range tr = {1, 1, 0, 1};
    rt_params pv = *p;
    pv.min_sample = pv.max_sample = 1;
    rt_status st = validate_render(s, &cam, &pv, &tr);
    if (st) return st;
    DeviceState *D = nullptr;
    if ((st = prepare_device(s, device, &D))) return st;
    if (n == 0) return RT_OK;
    DeviceClaim claim(D);
    if (!claim.ok) return fail(RT_ERR_STATE, "rt_shade_rays: another call on this scene is using device %d", device);
    if ((st = order_after_pending(D, D->stream))) return st;
    const size_t limit = chunk_samples_limit(true);
    const size_t chunk = (size_t)std::min<int64_t>(n, (int64_t)limit);
    const bool reproducible = (s->render_flags.load() & RT_RENDER_REPRODUCIBLE) != 0;
    if ((st = ensure_workspace(D, 0, chunk, pv.bounce, 1, 2, pv.caustic_k > 0 && D->scene.cm.n_leaves != 0, 0, 0, reproducible))) return st;
    const DevWork W = make_work(D, 0);
    RenderPass pass = {};
    camera_setup(cam, pass.cam);
    pass.ns = pass.max_sample = 1; pass.mode = 2;
    pass.fx = reproducible ? (unsigned long long *)D->ws[0].sample_fx.p : nullptr;     // run_pipeline folds it before the copy back
    HIP_TRY(stats_zero(W.stats, 0, ST_COUNT, D->stream));
    for (int64_t off = 0; off < n; off += (int64_t)chunk) {
        const uint32_t m = (uint32_t)std::min<int64_t>((int64_t)chunk, n - off);
        if ((st = D->t_in.upload(rays + 6 * off, (size_t)m * 24))) return st;
        HIP_TRY(hipMemsetAsync(W.sample_hit, 0, m, D->stream));
        HIP_TRY(hipMemsetAsync(W.sample_rgb, 0, (size_t)m * 12, D->stream));
        pass.q0 = (uint32_t)off; pass.npix = m; pass.rays = (const float *)D->t_in.p;      // (the upload above may have moved the buffer)
        if ((st = run_pipeline(D, D->stream, W, pv, nullptr, pass))) return st;
        HIP_TRY(hipStreamSynchronize(D->stream));
        HIP_TRY(hipMemcpy(hit + off, W.sample_hit, m, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(rgb + 3 * off, W.sample_rgb, (size_t)m * 12, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(z + off, W.sample_z, (size_t)m * 4, hipMemcpyDeviceToHost));
    }
    unsigned long long hs[ST_COUNT];
    HIP_TRY(stats_read(W.stats, 0, ST_COUNT, hs));
    if (hs[ST_QUEUE_OVERFLOW]) return fail(RT_ERR_LIMIT, "rt_shade_rays: queue overflow");
    for (int64_t i = 0; i < n; i++) if (!hit[i]) z[i] = 1.0e30f;
    return RT_OK;
}
