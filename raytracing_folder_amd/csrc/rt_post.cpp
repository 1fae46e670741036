// rt_post.cpp -- the image-space stages of the C ABI in include/rt_mi355x.h: denoising, temporal accumulation, motion vectors,
// exposure and tone mapping, bloom, motion blur, depth of field.  None of them knows a scene, but for the scene form of the motion
// vectors (rt_scene_motion: "motion vectors for deforming meshes", which walks a lowered scene's meshes).  Every stage is the same few steps -- check the
// versioned structs and the image size, find the device, order the stream behind the previous call on the same object, launch,
// record -- and its host entry point is the device one between an upload and a download; the pieces they share come first.
// There is no CPU path: without a gfx950 device the calls fail.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <vector>

#include "rt_host.h"

// ---- the shared skeleton --------------------------------------------------------------------------------------------------
// a versioned struct carries its caller's sizeof first
static rt_status check_struct(const char *name, const char *type, uint32_t given, size_t ours)
{
    if (given != (uint32_t)ours) return fail(RT_ERR_ARG, "%s: %s.struct_size is %u, this library's is %zu", name, type, given, ours);
    return RT_OK;
}
// the head of four stages' checks: both structs given, both of this library's size
template <class P, class L>
static rt_status check_params_planes(const char *name, const char *p_type, const P *p, const char *pl_type, const L *pl)
{
    if (!p || !pl) return fail(RT_ERR_ARG, "%s: params or planes is NULL", name);
    rt_status st = check_struct(name, p_type, p->struct_size, sizeof *p);
    return st ? st : check_struct(name, pl_type, pl->struct_size, sizeof *pl);
}

#define RT_IMAGE_MAX_PIXELS (1ll << 30)         /* 48 GiB of denoiser scratch; keeps the one-dimensional grid of 32 x 8 tiles far below 2^31 */
static rt_status check_image_dims(const char *name, int32_t w, int32_t h)
{
    return w <= 0 || h <= 0 ? fail(RT_ERR_ARG, "%s: bad image size %d x %d", name, w, h) : RT_OK;
}
static rt_status check_image_limit(const char *name, int32_t w, int32_t h)
{
    return (long long)w * h > RT_IMAGE_MAX_PIXELS ? fail(RT_ERR_LIMIT, "%s: %d x %d is more than 2^30 pixels", name, w, h) : RT_OK;
}
// both, where nothing is checked between them
static rt_status check_image_size(const char *name, int32_t w, int32_t h)
{
    rt_status st = check_image_dims(name, w, h);
    return st ? st : check_image_limit(name, w, h);
}

static rt_status need_gfx950(const char *name, int device)
{
    return device_is_gfx950(device) ? RT_OK : fail(RT_ERR_NO_DEVICE, "%s: device %d is not gfx950 (no CPU path)", name, device);
}

static bool planes_overlap(const void *a, size_t bytes_a, const void *b, size_t bytes_b)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + bytes_b && y < x + bytes_a;
}

// k_resolve's exponent is (float)(1.0 / gamma) of a DOUBLE gamma (rt_params); the stages' params carry a float.  Taking the
// double that prints like that float to 7 digits gives 2.2 for 2.2f, hence the exponent a default render used.
static float display_inv_gamma(float gamma)
{
    char buf[32];
    snprintf(buf, sizeof buf, "%.7g", (double)gamma);
    return (float)(1.0 / strtod(buf, nullptr));
}

namespace {                             // (internal linkage: the dynamic symbol table does not see these)
// What orders the calls that share one object or one device's scratch: each call makes its stream wait for the event the call
// before it recorded, whatever stream that one ran on, and records the event behind its own work.  The owner's mutex is held.
struct StageSync {
    Event done; bool pending = false;
    hipError_t create() { return done.create(hipEventDisableTiming); }
    rt_status wait(hipStream_t st) { if (pending) HIP_TRY(hipStreamWaitEvent(st, done, 0)); return RT_OK; }
    rt_status record(hipStream_t st) { HIP_TRY(hipEventRecord(done, st)); pending = true; return RT_OK; }
    // the end of a call: record, and a synchronous call leaves nothing pending
    rt_status settle(hipStream_t st, int sync)
    {
        rt_status rs = record(st);
        if (rs == RT_OK && sync) { HIP_TRY(hipStreamSynchronize(st)); pending = false; }
        return rs;
    }
    // on the host, before the owner's memory is overwritten or read back
    rt_status wait_host() { if (pending) { HIP_TRY(hipEventSynchronize(done)); pending = false; } return RT_OK; }
};

// The objects of the stages that keep state between frames (rt_history, rt_exposure, rt_bloom, rt_motion_blur, rt_dof) start like
// this; each adds its buffers and a release() that frees them.
struct StageObject {
    int device = 0; int32_t w = 0, h = 0;
    StageSync sync;
    std::mutex mu;
};
template <class T> static void stage_destroy(T *o)
{
    if (!o) return;
    if (hipSetDevice(o->device) == hipSuccess) {
        if (o->sync.pending) (void)hipEventSynchronize(o->sync.done);
        o->release();                   // hipFree waits for the kernels that still use the buffers
    }
    delete o;
}
// after the argument checks of a create: the device, the object, its buffers (`size` ensures them), its event
template <class T, class F> static rt_status stage_create(const char *name, int device, int32_t w, int32_t h, T **out, F size)
{
    rt_status st = need_gfx950(name, device);
    if (st) return st;
    HIP_TRY(hipSetDevice(device));
    T *o = new T;
    o->device = device; o->w = w; o->h = h;
    st = size(*o);
    if (st == RT_OK && o->sync.create() != hipSuccess) st = fail(RT_ERR_DEVICE, "%s: hipEventCreate failed", name);
    if (st) { stage_destroy(o); return st; }
    *out = o;
    return RT_OK;
}

// rt_denoise_device and rt_motion_device have no object, and the DeviceState of rt_host.h belongs to a scene: their scratch
// (a T with a release()) is held per device for the process, and every call on a device shares it under the registry's mutex.
// Released with the last scene (rt_scene_destroy), like the per-device buffers of the scenes.
template <class T> using PerDevice = std::vector<std::pair<int, T>>;
template <class T> static T &device_entry(PerDevice<T> &all, int device)      // under the registry's mutex
{
    for (auto &d : all) if (d.first == device) return d.second;
    all.emplace_back(device, T());
    return all.back().second;
}
template <class T> static void release_devices(std::mutex &mu, PerDevice<T> &all)
{
    std::lock_guard<std::mutex> lk(mu);
    for (auto &d : all)
        if (hipSetDevice(d.first) == hipSuccess) d.second.release();        // hipFree waits for the kernels that still use it
    all.clear();
}

// The round trip of a host entry point: its planes in device buffers that live as long as this does.  in() uploads a plane,
// out() makes room for one; both return a slot (-1 for a plane that is not given) and stop at the first failure, which `st`
// keeps.  An input whose buffer the stage overwrites in place names the host plane that receives it afterwards.
struct HostPlanes {
    enum { MAX = 12 };
    ScopedDevBuf buf[MAX]; void *back[MAX] = {}; size_t bytes[MAX] = {};
    int n = 0; rt_status st = RT_OK;
    int add(const void *src, void *dst, size_t nbytes)
    {
        if (st || !(src || dst)) return -1;
        st = src ? buf[n].upload(src, nbytes) : buf[n].ensure(nbytes);
        back[n] = dst; bytes[n] = nbytes;
        return n++;
    }
    int in(const void *host, size_t nbytes, void *in_place_out = nullptr) { return host ? add(host, in_place_out, nbytes) : -1; }
    int out(void *host, size_t nbytes) { return add(nullptr, host, nbytes); }
    template <class T> T *dev(int slot) const { return slot < 0 ? nullptr : (T *)buf[slot].p; }
    // ... as an output: NULL when the caller does not want that plane back
    template <class T> T *dev_out(int slot) const { return slot < 0 || !back[slot] ? nullptr : (T *)buf[slot].p; }
    // after the synchronous call: the wanted outputs among `slots`, in that order
    rt_status download(std::initializer_list<int> slots)
    {
        for (int s : slots)
            if (s >= 0 && back[s]) HIP_TRY(hipMemcpy(back[s], buf[s].p, bytes[s], hipMemcpyDeviceToHost));
        return RT_OK;
    }
};
}

// ---- denoising ----------------------------------------------------------------------------------------------------------
// The denoiser's scratch: the two ping-pong colour buffers and the guide buffer in one allocation, grown on demand.  Every
// denoise on a device uses the same scratch, so a call orders its stream behind the previous call's event.
namespace { struct DenoiseDevice { DevBuf scratch; StageSync sync; void release() { scratch.release(); } }; }
static std::mutex g_denoise_mu;
static PerDevice<DenoiseDevice> g_denoise;        // under g_denoise_mu

extern "C" void rt_denoise_default_params(rt_denoise_params *p)
{
    if (!p) return;
    p->struct_size = (uint32_t)sizeof *p;
    p->levels = 5; p->sigma_color = 1.0f; p->sigma_normal = 0.3f; p->sigma_depth = 0.05f; p->gamma = 2.2f;
}

extern "C" void rt_denoise_var_default(rt_denoise_var *v)
{
    if (!v) return;
    v->struct_size = (uint32_t)sizeof *v;
    v->variance = nullptr; v->out_variance = nullptr; v->k_sigma = 4.0f;
}

// everything that can be refused without a device, for every entry point; `v`: the variance block of the _var ones
static rt_status denoise_check(const char *name, int32_t w, int32_t h, const rt_denoise_params *p, const rt_denoise_planes *pl,
                               bool with_var = false, const rt_denoise_var *v = nullptr)
{
    rt_status st = check_params_planes(name, "rt_denoise_params", p, "rt_denoise_planes", pl);
    if (st || (st = check_image_dims(name, w, h))) return st;
    if (p->levels < 1 || p->levels > 8) return fail(RT_ERR_ARG, "%s: levels is %d, allowed 1..8", name, p->levels);
    for (float s : {p->sigma_color, p->sigma_normal, p->sigma_depth, p->gamma})
        if (!(s > 0.0f) || !std::isfinite(s)) return fail(RT_ERR_ARG, "%s: sigma_color, sigma_normal, sigma_depth and gamma must be positive and finite", name);
    if (!pl->rgb_linear || !pl->normal || !pl->albedo || !pl->z || !pl->out_linear)
        return fail(RT_ERR_ARG, "%s: rgb_linear, normal, albedo, z and out_linear are required", name);
    if ((st = check_image_limit(name, w, h)) || !with_var) return st;
    if (!v) return fail(RT_ERR_ARG, "%s: the variance block is NULL", name);
    if ((st = check_struct(name, "rt_denoise_var", v->struct_size, sizeof *v))) return st;
    if (!v->variance) return fail(RT_ERR_ARG, "%s: the variance plane is required", name);
    if (!(v->k_sigma > 0.0f) || !std::isfinite(v->k_sigma)) return fail(RT_ERR_ARG, "%s: k_sigma must be positive and finite", name);
    return RT_OK;
}

// v == NULL: the fixed-sigma filter; otherwise the variance-guided one (v is checked by the caller)
static rt_status denoise_on_device(const char *name, int device, hipStream_t st, int32_t w, int32_t h, const rt_denoise_params *p,
                                   const rt_denoise_planes *pl, int sync, const rt_denoise_var *v = nullptr)
{
    rt_status rs = need_gfx950(name, device);
    if (rs) return rs;
    HIP_TRY(hipSetDevice(device));
    std::lock_guard<std::mutex> lk(g_denoise_mu);
    DenoiseDevice &D = device_entry(g_denoise, device);
    const size_t n = (size_t)w * (size_t)h;
    // growing frees the old one, which waits for its users
    if ((rs = D.scratch.ensure(n * (v ? RT_DENOISE_SCRATCH_PER_PIXEL_VAR : RT_DENOISE_SCRATCH_PER_PIXEL)))) return rs;
    if (!D.sync.done) HIP_TRY(D.sync.create());
    if ((rs = D.sync.wait(st))) return rs;
    DenoiseRequest R = {};
    R.width = w; R.height = h; R.levels = p->levels;
    R.sigma_color = p->sigma_color; R.sigma_normal = p->sigma_normal; R.sigma_depth = p->sigma_depth; R.inv_gamma = display_inv_gamma(p->gamma);
    R.rgb_linear = pl->rgb_linear; R.normal = pl->normal; R.albedo = pl->albedo; R.z = pl->z; R.object_id = pl->object_id;
    R.out_linear = pl->out_linear; R.out_rgb8 = pl->out_rgb8;
    R.color[0] = (float4 *)D.scratch.p; R.color[1] = R.color[0] + n; R.guide = R.color[1] + n;
    if (v) {
        R.variance = v->variance; R.out_variance = v->out_variance; R.k_sigma = v->k_sigma;
        R.var[0] = R.guide + n; R.var[1] = R.var[0] + n;
    }
    rtk_launch_denoise_frame(st, R);
    HIP_TRY(hipGetLastError());
    return D.sync.settle(st, sync);
}

// rt_denoise and rt_denoise_var_host: upload, filter, download.  The results are written in place into the uploaded planes
static rt_status denoise_host(const char *name, int device, int32_t w, int32_t h, const rt_denoise_params *p, const rt_denoise_planes *pl,
                              bool with_var, const rt_denoise_var *v)
{
    rt_status st = denoise_check(name, w, h, p, pl, with_var, v);
    if (st || (st = need_gfx950(name, device))) return st;
    HIP_TRY(hipSetDevice(device));
    const size_t n = (size_t)w * (size_t)h;
    HostPlanes S;
    const int rgb = S.in(pl->rgb_linear, n * 12, pl->out_linear), normal = S.in(pl->normal, n * 12), albedo = S.in(pl->albedo, n * 12), z = S.in(pl->z, n * 4);
    const int var = v ? S.in(v->variance, n * 12, v->out_variance) : -1;
    const int id = S.in(pl->object_id, n * 4), rgb8 = S.out(pl->out_rgb8, n * 3);
    if (S.st) return S.st;
    const rt_denoise_planes dev = {(uint32_t)sizeof dev, S.dev<float>(rgb), S.dev<float>(normal), S.dev<float>(albedo), S.dev<float>(z),
                                   S.dev<int32_t>(id), S.dev<float>(rgb), S.dev<uint8_t>(rgb8)};
    rt_denoise_var dv;
    if (v) dv = {(uint32_t)sizeof dv, S.dev<float>(var), S.dev_out<float>(var), v->k_sigma};
    if ((st = denoise_on_device(name, device, nullptr, w, h, p, &dev, 1, v ? &dv : nullptr))) return st;
    return S.download({rgb, rgb8, var});
}

extern "C" rt_status rt_denoise_device(int device, void *hip_stream, int32_t w, int32_t h, const rt_denoise_params *p,
                                       const rt_denoise_planes *device_planes, int sync)
{
    rt_status st = denoise_check("rt_denoise_device", w, h, p, device_planes);
    return st ? st : denoise_on_device("rt_denoise_device", device, (hipStream_t)hip_stream, w, h, p, device_planes, sync);
}

extern "C" rt_status rt_denoise(int device, int32_t w, int32_t h, const rt_denoise_params *p, const rt_denoise_planes *host_planes)
{
    return denoise_host("rt_denoise", device, w, h, p, host_planes, false, nullptr);
}

extern "C" rt_status rt_denoise_var_device(int device, void *hip_stream, int32_t w, int32_t h, const rt_denoise_params *p,
                                           const rt_denoise_planes *device_planes, const rt_denoise_var *v, int sync)
{
    rt_status st = denoise_check("rt_denoise_var_device", w, h, p, device_planes, true, v);
    return st ? st : denoise_on_device("rt_denoise_var_device", device, (hipStream_t)hip_stream, w, h, p, device_planes, sync, v);
}

extern "C" rt_status rt_denoise_var_host(int device, int32_t w, int32_t h, const rt_denoise_params *p, const rt_denoise_planes *host_planes,
                                         const rt_denoise_var *v)
{
    return denoise_host("rt_denoise_var_host", device, w, h, p, host_planes, true, v);
}

// ---- temporal accumulation ----------------------------------------------------------------------------------------------
// An rt_history owns what one stream of frames needs on its device: the two ping-pong sets in one allocation, the camera of the
// frame the current set holds, and the event that orders a call behind the previous one on the same history.
struct rt_history : StageObject {
    DevBuf sets;                        // RT_TEMPORAL_HISTORY_PER_PIXEL bytes a pixel: set 0, set 1
    int cur = 0;                        // the set the last frame wrote
    int32_t frames = 0;                 // since create / reset; 0: the next frame reads no history
    DevCamera cam = {};                 // of the frame in set `cur`
    DevBuf clip_out;                    // rt_temporal_clip_device with out_linear over rgb_linear: 12 bytes a pixel, made on first use
    void release() { sets.release(); clip_out.release(); }
};

extern "C" rt_status rt_history_create(int device, int32_t w, int32_t h, rt_history **out)
{
    if (!out) return fail(RT_ERR_ARG, "rt_history_create: out is NULL");
    *out = nullptr;
    rt_status st = check_image_size("rt_history_create", w, h);
    if (st) return st;
    return stage_create("rt_history_create", device, w, h, out,
                        [](rt_history &hst) { return hst.sets.ensure((size_t)hst.w * (size_t)hst.h * RT_TEMPORAL_HISTORY_PER_PIXEL); });
}

extern "C" rt_status rt_history_reset(rt_history *hst)
{
    if (!hst) return fail(RT_ERR_ARG, "rt_history_reset: history is NULL");
    std::lock_guard<std::mutex> lk(hst->mu);
    hst->frames = 0;                    // the next frame reads no tap; it still waits for the event before it writes a set
    return RT_OK;
}

extern "C" void rt_history_destroy(rt_history *hst) { stage_destroy(hst); }

extern "C" int32_t rt_history_frames(const rt_history *hst) { return hst ? hst->frames : 0; }

extern "C" void rt_temporal_default_params(rt_temporal_params *p)
{
    if (!p) return;
    p->struct_size = (uint32_t)sizeof *p;
    p->alpha = 0.2f; p->max_history = 32; p->sigma_normal = 0.3f; p->sigma_depth = 0.05f; p->gamma = 2.2f;
}

// everything that can be refused without a device, for every entry point; the history comes last, so that a caller without a
// device (which has no history) is told about its other arguments too
static rt_status temporal_check(const char *name, const rt_history *hst, const rt_camera *cam, const rt_temporal_params *p, const rt_temporal_planes *pl)
{
    if (!cam || !p || !pl) return fail(RT_ERR_ARG, "%s: camera, params or planes is NULL", name);
    rt_status st = check_struct(name, "rt_temporal_params", p->struct_size, sizeof *p);
    if (st || (st = check_struct(name, "rt_temporal_planes", pl->struct_size, sizeof *pl))) return st;
    if (!(p->alpha > 0.0f && p->alpha <= 1.0f)) return fail(RT_ERR_ARG, "%s: alpha must be in (0, 1]", name);
    if (p->max_history < 1 || p->max_history > 65535) return fail(RT_ERR_ARG, "%s: max_history is %d, allowed 1..65535", name, p->max_history);
    for (float s : {p->sigma_normal, p->sigma_depth, p->gamma})
        if (!(s > 0.0f) || !std::isfinite(s)) return fail(RT_ERR_ARG, "%s: sigma_normal, sigma_depth and gamma must be positive and finite", name);
    if (!pl->rgb_linear || !pl->normal || !pl->albedo || !pl->z || !pl->out_linear)
        return fail(RT_ERR_ARG, "%s: rgb_linear, normal, albedo, z and out_linear are required", name);
    if (pl->out_variance && !pl->variance) return fail(RT_ERR_ARG, "%s: out_variance needs the variance plane", name);
    if (!hst) return fail(RT_ERR_ARG, "%s: history is NULL", name);
    if (cam->width != hst->w || cam->height != hst->h)
        return fail(RT_ERR_ARG, "%s: the camera is %d x %d, the history %d x %d", name, cam->width, cam->height, hst->w, hst->h);
    return RT_OK;
}

extern "C" void rt_temporal_clip_default(rt_temporal_clip *c)
{
    if (!c) return;
    c->struct_size = (uint32_t)sizeof *c;
    c->radius = 2; c->k_clip = 1.5f; c->min_count = 4; c->clip_history = 2; c->out_clipped = nullptr;
}

// what rt_temporal_clip_* check before temporal_check, without a device
static rt_status temporal_clip_check(const char *name, const rt_temporal_clip *c)
{
    if (!c) return fail(RT_ERR_ARG, "%s: the rt_temporal_clip is NULL", name);
    rt_status st = check_struct(name, "rt_temporal_clip", c->struct_size, sizeof *c);
    if (st) return st;
    if (c->radius < 1 || c->radius > 3) return fail(RT_ERR_ARG, "%s: radius is %d, allowed 1..3", name, c->radius);
    if (!(c->k_clip > 0.0f) || !std::isfinite(c->k_clip)) return fail(RT_ERR_ARG, "%s: k_clip must be positive and finite", name);
    if (c->min_count < 1) return fail(RT_ERR_ARG, "%s: min_count is %d, allowed >= 1", name, c->min_count);
    if (c->clip_history < 1 || c->clip_history > 65535) return fail(RT_ERR_ARG, "%s: clip_history is %d, allowed 1..65535", name, c->clip_history);
    return RT_OK;
}

// motion: NULL (reproject with the two cameras), or the device plane of rt_motion_device for this frame.  clip: NULL (k_temporal),
// or the validated rectification (k_temporal_clip), its out_clipped a device plane
static rt_status temporal_on_device(rt_history *hst, hipStream_t st, const rt_camera *cam, const rt_temporal_params *p, const rt_temporal_planes *pl, int sync,
                                    const float *motion = nullptr, const rt_temporal_clip *clip = nullptr)
{
    HIP_TRY(hipSetDevice(hst->device));
    std::lock_guard<std::mutex> lk(hst->mu);
    rt_status rs = hst->sync.wait(st);
    if (rs) return rs;
    const size_t n = (size_t)hst->w * (size_t)hst->h;
    TemporalRequest R = {};
    R.width = hst->w; R.height = hst->h; R.has_history = hst->frames > 0;
    camera_setup(*cam, R.cur);
    R.old = hst->cam;
    R.alpha = p->alpha; R.max_history = p->max_history; R.sigma_normal = p->sigma_normal; R.sigma_depth = p->sigma_depth;
    R.inv_gamma = display_inv_gamma(p->gamma);
    R.rgb_linear = pl->rgb_linear; R.normal = pl->normal; R.albedo = pl->albedo; R.z = pl->z; R.object_id = pl->object_id; R.variance = pl->variance;
    R.out_linear = pl->out_linear; R.out_variance = pl->out_variance; R.out_history = pl->out_history; R.out_rgb8 = pl->out_rgb8;
    float4 *set0 = (float4 *)hst->sets.p;
    const int next = hst->cur ^ 1;
    R.prev = set0 + (size_t)hst->cur * 3 * n; R.next = set0 + (size_t)next * 3 * n;
    R.motion = motion;
    if (clip) {
        // k_temporal_clip's workgroups read their neighbours' pixels of rgb_linear: where out_linear overlaps it, the kernel writes
        // a plane of the history's and the result is copied behind it on the same stream
        const bool overlap = planes_overlap(pl->rgb_linear, n * 12, pl->out_linear, n * 12);
        if (overlap) {
            if ((rs = hst->clip_out.ensure(n * 12))) return rs;
            R.out_linear = (float *)hst->clip_out.p;
        }
        TemporalClipRequest CR = {};
        CR.frame = R;
        CR.radius = clip->radius; CR.min_count = clip->min_count; CR.k_clip = clip->k_clip; CR.clip_history = clip->clip_history;
        CR.out_clipped = clip->out_clipped;
        rtk_launch_temporal_clip(st, CR);
        HIP_TRY(hipGetLastError());
        if (overlap) HIP_TRY(hipMemcpyAsync(pl->out_linear, hst->clip_out.p, n * 12, hipMemcpyDeviceToDevice, st));
    } else {
        rtk_launch_temporal(st, R);
    }
    HIP_TRY(hipGetLastError());
    if ((rs = hst->sync.record(st))) return rs;
    hst->cur = next; hst->cam = R.cur; hst->frames++;
    if (sync) { HIP_TRY(hipStreamSynchronize(st)); hst->sync.pending = false; }
    return RT_OK;
}

// the host entry points: upload, accumulate, download.  motion: NULL (rt_temporal), or this frame's plane on the host.  The
// results are written in place into the uploaded colour and variance
static rt_status temporal_host(const char *name, rt_history *hst, const rt_camera *cam, const rt_temporal_params *p, const rt_temporal_planes *pl,
                               const float *motion, const rt_temporal_clip *clip = nullptr)
{
    rt_status st = temporal_check(name, hst, cam, p, pl);
    if (st) return st;
    HIP_TRY(hipSetDevice(hst->device));
    const size_t n = (size_t)hst->w * (size_t)hst->h;
    HostPlanes S;
    const int rgb = S.in(pl->rgb_linear, n * 12, pl->out_linear), normal = S.in(pl->normal, n * 12), albedo = S.in(pl->albedo, n * 12), z = S.in(pl->z, n * 4);
    const int id = S.in(pl->object_id, n * 4), var = S.in(pl->variance, n * 12, pl->out_variance), mv = S.in(motion, n * 12);
    const int hist = S.out(pl->out_history, n * 4), rgb8 = S.out(pl->out_rgb8, n * 3);
    const int mask = clip ? S.out(clip->out_clipped, n * 4) : -1;
    if (S.st) return S.st;
    const rt_temporal_planes dev = {(uint32_t)sizeof dev, S.dev<float>(rgb), S.dev<float>(normal), S.dev<float>(albedo), S.dev<float>(z),
                                    S.dev<int32_t>(id), S.dev<float>(var), S.dev<float>(rgb),
                                    S.dev_out<float>(var), S.dev<float>(hist), S.dev<uint8_t>(rgb8)};
    rt_temporal_clip dev_clip;
    if (clip) { dev_clip = *clip; dev_clip.out_clipped = S.dev<float>(mask); }
    if ((st = temporal_on_device(hst, nullptr, cam, p, &dev, 1, S.dev<float>(mv), clip ? &dev_clip : nullptr))) return st;
    return S.download({mask, rgb, var, hist, rgb8});
}

extern "C" rt_status rt_temporal_device(rt_history *hst, void *hip_stream, const rt_camera *cam, const rt_temporal_params *p,
                                        const rt_temporal_planes *device_planes, int sync)
{
    rt_status st = temporal_check("rt_temporal_device", hst, cam, p, device_planes);
    return st ? st : temporal_on_device(hst, (hipStream_t)hip_stream, cam, p, device_planes, sync);
}

extern "C" rt_status rt_temporal(rt_history *hst, const rt_camera *cam, const rt_temporal_params *p, const rt_temporal_planes *host_planes)
{
    return temporal_host("rt_temporal", hst, cam, p, host_planes, nullptr);
}

extern "C" rt_status rt_temporal_motion_device(rt_history *hst, void *hip_stream, const rt_camera *cam, const rt_temporal_params *p,
                                               const rt_temporal_planes *device_planes, const float *motion_dev, int sync)
{
    if (!motion_dev) return fail(RT_ERR_ARG, "rt_temporal_motion_device: the motion plane is NULL");
    rt_status st = temporal_check("rt_temporal_motion_device", hst, cam, p, device_planes);
    return st ? st : temporal_on_device(hst, (hipStream_t)hip_stream, cam, p, device_planes, sync, motion_dev);
}

extern "C" rt_status rt_temporal_motion(rt_history *hst, const rt_camera *cam, const rt_temporal_params *p, const rt_temporal_planes *host_planes,
                                        const float *motion)
{
    if (!motion) return fail(RT_ERR_ARG, "rt_temporal_motion: the motion plane is NULL");
    return temporal_host("rt_temporal_motion", hst, cam, p, host_planes, motion);
}

extern "C" rt_status rt_temporal_clip_device(rt_history *hst, void *hip_stream, const rt_camera *cam, const rt_temporal_params *p,
                                             const rt_temporal_clip *clip, const rt_temporal_planes *device_planes, const float *motion_dev, int sync)
{
    rt_status st = temporal_clip_check("rt_temporal_clip_device", clip);
    if (st) return st;
    if ((st = temporal_check("rt_temporal_clip_device", hst, cam, p, device_planes))) return st;
    return temporal_on_device(hst, (hipStream_t)hip_stream, cam, p, device_planes, sync, motion_dev, clip);
}

extern "C" rt_status rt_temporal_clip_host(rt_history *hst, const rt_camera *cam, const rt_temporal_params *p, const rt_temporal_clip *clip,
                                           const rt_temporal_planes *host_planes, const float *motion)
{
    rt_status st = temporal_clip_check("rt_temporal_clip_host", clip);
    return st ? st : temporal_host("rt_temporal_clip_host", hst, cam, p, host_planes, motion, clip);
}

// ---- motion vectors ---------------------------------------------------------------------------------------------------------
// One affine map in double, X -> r X + t (r row-major), and the two steps the node chains are made of.
namespace {
struct Affine64 {
    double r[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
    // this, then M X + c (M column-major float[9], like rt_node's)
    Affine64 then(const float *M, const double c[3]) const
    {
        Affine64 o;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) o.r[3 * i + j] = (double)M[i] * r[j] + (double)M[3 + i] * r[3 + j] + (double)M[6 + i] * r[6 + j];
            o.t[i] = (double)M[i] * t[0] + (double)M[3 + i] * t[1] + (double)M[6 + i] * t[2] + c[i];
        }
        return o;
    }
    // this, then A
    Affine64 then(const Affine64 &A) const
    {
        Affine64 o;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) o.r[3 * i + j] = A.r[3 * i] * r[j] + A.r[3 * i + 1] * r[3 + j] + A.r[3 * i + 2] * r[6 + j];
            o.t[i] = A.r[3 * i] * t[0] + A.r[3 * i + 1] * t[1] + A.r[3 * i + 2] * t[2] + A.t[i];
        }
        return o;
    }
};
}

// The table of rt_motion: per node i the map A_i of this frame's world into the previous frame's -- TransformTo down the chain
// root .. i of `nodes` (per node itm (X - pos)), then TransformFrom up the chain i .. root of `prev` (per node tm X + pos) --
// composed in double and rounded to float once.  A node whose chain is bit-identical in both arrays (and every node when prev
// is NULL) gets exactly the identity.  The parents were validated by the caller.
static void motion_table(const rt_node *nodes, const rt_node *prev, int32_t n, std::vector<DevNodeMotion> &table)
{
    table.resize((size_t)n);
    std::vector<Affine64> to, from;     // world -> node i down the current chain; node i -> world up the previous chain
    std::vector<char> same((size_t)n, 1);
    if (prev) { to.resize((size_t)n); from.resize((size_t)n); }
    for (int32_t i = 0; i < n; i++) {
        Affine64 A;
        if (prev) {
            const rt_node &c = nodes[i], &o = prev[i];
            same[i] = c.parent == o.parent && !memcmp(c.tm, o.tm, 36) && !memcmp(c.itm, o.itm, 36) && !memcmp(c.pos, o.pos, 12) &&
                      (c.parent < 0 || same[c.parent]);
            double mp[3];               // itm (X - pos) = itm X - itm pos
            for (int k = 0; k < 3; k++) mp[k] = -((double)c.itm[k] * c.pos[0] + (double)c.itm[3 + k] * c.pos[1] + (double)c.itm[6 + k] * c.pos[2]);
            to[i] = (c.parent < 0 ? Affine64() : to[c.parent]).then(c.itm, mp);
            const double op[3] = {o.pos[0], o.pos[1], o.pos[2]};
            const Affine64 up = Affine64().then(o.tm, op);
            from[i] = o.parent < 0 ? up : up.then(from[o.parent]);
            if (!same[i]) A = to[i].then(from[i]);
        }
        for (int k = 0; k < 3; k++) table[i].row[k] = make_float4((float)A.r[3 * k], (float)A.r[3 * k + 1], (float)A.r[3 * k + 2], (float)A.t[k]);
    }
}

// everything that can be refused without a device, for both entry points
static rt_status motion_check(const char *name, const rt_camera *cam, const rt_camera *prev_cam, const rt_node *nodes, const rt_node *prev_nodes,
                              int32_t n_nodes, const rt_motion_planes *pl)
{
    if (!cam || !prev_cam || !nodes || !pl) return fail(RT_ERR_ARG, "%s: camera, prev_cam, nodes or planes is NULL", name);
    rt_status st = check_struct(name, "rt_motion_planes", pl->struct_size, sizeof *pl);
    if (st) return st;
    if (!pl->z || !pl->object_id || !pl->motion) return fail(RT_ERR_ARG, "%s: z, object_id and motion are required", name);
    if (n_nodes <= 0) return fail(RT_ERR_ARG, "%s: n_nodes is %d", name, n_nodes);
    for (const rt_node *arr : {nodes, prev_nodes})
        for (int32_t i = 0; arr && i < n_nodes; i++)
            if (arr[i].parent < -1 || arr[i].parent >= i)
                return fail(RT_ERR_ARG, "%s: node %d of %s has parent %d (a parent must precede its child; -1: none)", name, i,
                            arr == nodes ? "nodes" : "prev_nodes", arr[i].parent);
    if ((st = check_image_dims(name, cam->width, cam->height))) return st;
    if (cam->width != prev_cam->width || cam->height != prev_cam->height)
        return fail(RT_ERR_ARG, "%s: the camera is %d x %d, the previous one %d x %d", name, cam->width, cam->height, prev_cam->width, prev_cam->height);
    return check_image_limit(name, cam->width, cam->height);
}

// The node table of the last rt_motion call per device: kept between calls (a frame's table is uploaded only when it differs
// from the one the device holds).  Every call on the device shares it, so -- like the denoiser's scratch -- every call orders its
// stream behind the previous call's event, whatever that call's stream was and whether or not the table changes: the event
// then stands for ALL earlier calls, and waiting for it on the host before an overwrite leaves no kernel that still reads the
// table.
// rt_scene_motion_device keeps two more tables beside it under the same discipline -- the previous chains' object-to-world maps
// and the per-node mesh records -- and, for a scene whose trees can outgrow the LDS stack, k_motion_mesh's spill buffer.
namespace {
struct MotionDevice {
    DevBuf table, from, mesh_nodes, spill;
    std::vector<DevNodeMotion> held, held_from;
    std::vector<DevMotionMeshNode> held_mesh;
    StageSync sync;
    void release() { for (DevBuf *b : {&table, &from, &mesh_nodes, &spill}) b->release(); held.clear(); held_from.clear(); held_mesh.clear(); }
};
}
static std::mutex g_motion_mu;
static PerDevice<MotionDevice> g_motion;          // under g_motion_mu

void post_release_all()
{
    release_devices(g_denoise_mu, g_denoise);
    release_devices(g_motion_mu, g_motion);
}

rt_status motion_wait_host(int device)
{
    std::lock_guard<std::mutex> lk(g_motion_mu);
    for (auto &d : g_motion) if (d.first == device) return d.second.sync.wait_host();
    return RT_OK;
}

// a call's table onto the device when it differs from the one held there (the caller holds g_motion_mu and has made its stream
// wait for sync's event: waiting for that event on the host leaves no kernel that still reads the table)
template <class T> static rt_status motion_upload_if_different(DevBuf &buf, std::vector<T> &held, const std::vector<T> &table, StageSync &sync)
{
    const size_t bytes = table.size() * sizeof(T);
    if (held.size() == table.size() && memcmp(held.data(), table.data(), bytes) == 0) return RT_OK;
    rt_status rs = sync.wait_host();
    if (rs) return rs;
    held.clear();
    if ((rs = buf.upload(table.data(), bytes))) return rs;
    held = table;
    return RT_OK;
}

static rt_status motion_on_device(const char *name, int device, hipStream_t st, const rt_camera *cam, const rt_camera *prev_cam, const rt_node *nodes,
                                  const rt_node *prev_nodes, int32_t n_nodes, const rt_motion_planes *pl, int sync)
{
    rt_status rs = need_gfx950(name, device);
    if (rs) return rs;
    HIP_TRY(hipSetDevice(device));
    std::vector<DevNodeMotion> table;
    motion_table(nodes, prev_nodes, n_nodes, table);
    std::lock_guard<std::mutex> lk(g_motion_mu);
    MotionDevice &D = device_entry(g_motion, device);
    if (!D.sync.done) HIP_TRY(D.sync.create());
    if ((rs = D.sync.wait(st))) return rs;
    if ((rs = motion_upload_if_different(D.table, D.held, table, D.sync))) return rs;
    MotionRequest R = {};
    R.width = cam->width; R.height = cam->height; R.n_nodes = n_nodes;
    camera_setup(*cam, R.cur);
    camera_setup(*prev_cam, R.old);
    R.z = pl->z; R.object_id = pl->object_id; R.table = (const DevNodeMotion *)D.table.p; R.motion = pl->motion;
    rtk_launch_motion(st, R);
    HIP_TRY(hipGetLastError());
    return D.sync.settle(st, sync);
}

extern "C" rt_status rt_motion_device(int device, void *hip_stream, const rt_camera *cam, const rt_camera *prev_cam, const rt_node *nodes,
                                      const rt_node *prev_nodes, int32_t n_nodes, const rt_motion_planes *device_planes, int sync)
{
    rt_status st = motion_check("rt_motion_device", cam, prev_cam, nodes, prev_nodes, n_nodes, device_planes);
    return st ? st : motion_on_device("rt_motion_device", device, (hipStream_t)hip_stream, cam, prev_cam, nodes, prev_nodes, n_nodes, device_planes, sync);
}

extern "C" rt_status rt_motion(int device, const rt_camera *cam, const rt_camera *prev_cam, const rt_node *nodes, const rt_node *prev_nodes,
                               int32_t n_nodes, const rt_motion_planes *host_planes)
{
    rt_status st = motion_check("rt_motion", cam, prev_cam, nodes, prev_nodes, n_nodes, host_planes);
    if (st || (st = need_gfx950("rt_motion", device))) return st;
    HIP_TRY(hipSetDevice(device));
    const size_t n = (size_t)cam->width * (size_t)cam->height;
    HostPlanes S;
    const int z = S.in(host_planes->z, n * 4), id = S.in(host_planes->object_id, n * 4), mv = S.out(host_planes->motion, n * 12);
    if (S.st) return S.st;
    const rt_motion_planes dev = {(uint32_t)sizeof dev, S.dev<float>(z), S.dev<int32_t>(id), S.dev<float>(mv)};
    if ((st = motion_on_device("rt_motion", device, nullptr, cam, prev_cam, nodes, prev_nodes, n_nodes, &dev, 1))) return st;
    return S.download({mv});
}

// ---- motion vectors for deforming meshes ------------------------------------------------------------------------------------
// The one image-space stage that knows a scene: the pixels of a mesh that holds previous positions are traced (rt_motion_mesh.hip).
// The second table: per node i the object-to-world map up the chain i .. root of `nodes` (per node tm X + pos), composed in double
// and rounded to float once.  The parents were validated by the caller.
static void motion_from_table(const rt_node *nodes, int32_t n, std::vector<DevNodeMotion> &table)
{
    table.resize((size_t)n);
    std::vector<Affine64> from((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        const rt_node &o = nodes[i];
        const double op[3] = {o.pos[0], o.pos[1], o.pos[2]};
        const Affine64 up = Affine64().then(o.tm, op);
        const Affine64 &A = from[i] = o.parent < 0 ? up : up.then(from[o.parent]);
        for (int k = 0; k < 3; k++) table[i].row[k] = make_float4((float)A.r[3 * k], (float)A.r[3 * k + 1], (float)A.r[3 * k + 2], (float)A.t[k]);
    }
}

// everything that can be refused without a device, for both entry points; leaves the scene's nodes in `nodes`
static rt_status scene_motion_check(const char *name, rt_scene *s, int shade_model, const rt_camera *cam, const rt_camera *prev_cam, const rt_node *prev_nodes,
                                    int32_t n_nodes, float depth_tol, const rt_motion_planes *pl, std::vector<rt_node> &nodes)
{
    if (!s) return fail(RT_ERR_ARG, "%s: the scene is NULL", name);
    if (shade_model < RT_SHADE_FIN || shade_model > RT_SHADE_P3) return fail(RT_ERR_ARG, "%s: unknown shading model %d", name, shade_model);
    {
        std::lock_guard<std::mutex> lk(s->mu);
        nodes = s->data.nodes;
    }
    if (n_nodes <= 0 || (size_t)n_nodes != nodes.size()) return fail(RT_ERR_ARG, "%s: n_nodes is %d, the scene has %zu nodes", name, n_nodes, nodes.size());
    rt_status st = motion_check(name, cam, prev_cam, nodes.data(), prev_nodes, n_nodes, pl);
    if (st) return st;
    if (!(depth_tol > 0.0f) || !std::isfinite(depth_tol)) return fail(RT_ERR_ARG, "%s: depth_tol must be positive and finite", name);
    return check_idle(s, name);
}

static rt_status scene_motion_on_device(const char *name, rt_scene *s, int shade_model, int device, hipStream_t st, const rt_camera *cam, const rt_camera *prev_cam,
                                        const std::vector<rt_node> &nodes, const rt_node *prev_nodes, float depth_tol, const rt_motion_planes *pl, int sync)
{
    DeviceState *DS = nullptr;
    rt_status rs = prepare_device(s, device, &DS);        // (device range, gfx950, hipSetDevice; lowers the scene if it is not there)
    if (rs) return rs;
    DeviceClaim claim(DS);
    if (!claim.ok) return fail(RT_ERR_STATE, "%s: another call on this scene is using device %d", name, device);
    if (DS->last_pending && DS->last_done) HIP_TRY(hipEventSynchronize(DS->last_done));
    const int32_t n_nodes = (int32_t)nodes.size();
    if (DS->scene.n_nodes != n_nodes || DS->node_object.size() != nodes.size())
        return fail(RT_ERR_STATE, "%s: device %d does not hold the scene as it is now", name, device);
    std::vector<DevNodeMotion> table, from;
    motion_table(nodes.data(), prev_nodes, n_nodes, table);
    motion_from_table(prev_nodes ? prev_nodes : nodes.data(), n_nodes, from);
    // a node is a mesh node while its mesh holds previous positions on this device (they follow the store: rt_lower.cpp, rt_mesh_update.cpp)
    std::vector<DevMotionMeshNode> mesh_nodes((size_t)n_nodes);
    for (int32_t i = 0; i < n_nodes; i++) {
        DevMotionMeshNode &m = mesh_nodes[i];
        m.object = m.mesh = -1; m.v_prev = nullptr; m.slot_idx = nullptr;
        const rt_node &n = nodes[i];
        if (n.obj_type != RT_OBJ_MESH || DS->node_object[i] < 0 || n.mesh < 0 || (size_t)n.mesh >= DS->mesh_bufs.size()) continue;
        const DevMeshBufs &mb = DS->mesh_bufs[n.mesh];
        if (!mb.v_prev.p) continue;
        m.object = DS->node_object[i]; m.mesh = n.mesh;
        m.v_prev = (const float *)mb.v_prev.p; m.slot_idx = (const uint32_t *)mb.slot_idx.p;
    }
    std::lock_guard<std::mutex> lk(g_motion_mu);
    MotionDevice &D = device_entry(g_motion, device);
    if (!D.sync.done) HIP_TRY(D.sync.create());
    if ((rs = D.sync.wait(st))) return rs;
    if ((rs = motion_upload_if_different(D.table, D.held, table, D.sync)) || (rs = motion_upload_if_different(D.from, D.held_from, from, D.sync)) ||
        (rs = motion_upload_if_different(D.mesh_nodes, D.held_mesh, mesh_nodes, D.sync))) return rs;
    MotionMeshRequest R = {};
    R.rigid.width = cam->width; R.rigid.height = cam->height; R.rigid.n_nodes = n_nodes;
    camera_setup(*cam, R.rigid.cur);
    camera_setup(*prev_cam, R.rigid.old);
    R.rigid.z = pl->z; R.rigid.object_id = pl->object_id; R.rigid.table = (const DevNodeMotion *)D.table.p; R.rigid.motion = pl->motion;
    R.S = DS->scene;
    R.mesh_nodes = (const DevMotionMeshNode *)D.mesh_nodes.p; R.from = (const DevNodeMotion *)D.from.p;
    R.depth_tol = depth_tol; R.p13 = shade_model != RT_SHADE_FIN;
    // the traversal stack behind the LDS part: this stage's own, because a call that does not synchronise outlives its claim on
    // the scene's device state (whose spill buffer the single-stage entry points use)
    if (DS->scene.max_bvh_depth > RT_BVH_STACK) {
        if ((rs = D.spill.ensure(SPILL_BYTES))) return rs;
        R.spill = (uint32_t *)D.spill.p;
    }
    rtk_launch_motion_mesh(st, R);
    HIP_TRY(hipGetLastError());
    return D.sync.settle(st, sync);
}

extern "C" rt_status rt_scene_motion_device(rt_scene *s, int shade_model, int device, void *hip_stream, const rt_camera *cam, const rt_camera *prev_cam,
                                            const rt_node *prev_nodes, int32_t n_nodes, float depth_tol, const rt_motion_planes *device_planes, int sync)
{
    std::vector<rt_node> nodes;
    rt_status st = scene_motion_check("rt_scene_motion_device", s, shade_model, cam, prev_cam, prev_nodes, n_nodes, depth_tol, device_planes, nodes);
    return st ? st : scene_motion_on_device("rt_scene_motion_device", s, shade_model, device, (hipStream_t)hip_stream, cam, prev_cam, nodes, prev_nodes, depth_tol, device_planes, sync);
}

extern "C" rt_status rt_scene_motion(rt_scene *s, int shade_model, int device, const rt_camera *cam, const rt_camera *prev_cam, const rt_node *prev_nodes,
                                     int32_t n_nodes, float depth_tol, const rt_motion_planes *host_planes)
{
    std::vector<rt_node> nodes;
    rt_status st = scene_motion_check("rt_scene_motion", s, shade_model, cam, prev_cam, prev_nodes, n_nodes, depth_tol, host_planes, nodes);
    if (st || (st = need_gfx950("rt_scene_motion", device))) return st;
    HIP_TRY(hipSetDevice(device));
    const size_t n = (size_t)cam->width * (size_t)cam->height;
    HostPlanes S;
    const int z = S.in(host_planes->z, n * 4), id = S.in(host_planes->object_id, n * 4), mv = S.out(host_planes->motion, n * 12);
    if (S.st) return S.st;
    const rt_motion_planes dev = {(uint32_t)sizeof dev, S.dev<float>(z), S.dev<int32_t>(id), S.dev<float>(mv)};
    if ((st = scene_motion_on_device("rt_scene_motion", s, shade_model, device, nullptr, cam, prev_cam, nodes, prev_nodes, depth_tol, &dev, 1))) return st;
    return S.download({mv});
}

// ---- exposure and tone mapping --------------------------------------------------------------------------------------------
// An rt_exposure owns the device block of one stream of frames (ToneMapRequest::State) and the event that orders a call behind
// the previous one on the same state.  The host keeps no copy of what the meter computes: the getters read the block back.
struct rt_exposure : StageObject {      // (not tied to an image size: w and h stay 0)
    DevBuf block;                       // one ToneMapRequest::State
    void release() { block.release(); }
};

// the block back to all zero (an empty working histogram, no metered frame), behind the calls issued so far
static rt_status exposure_clear(rt_exposure *e)
{
    rt_status rs = e->sync.wait(nullptr);
    if (rs) return rs;
    HIP_TRY(hipMemsetAsync(e->block.p, 0, sizeof(ToneMapRequest::State), nullptr));
    return e->sync.record(nullptr);
}

extern "C" rt_status rt_exposure_create(int device, rt_exposure **out)
{
    if (!out) return fail(RT_ERR_ARG, "rt_exposure_create: out is NULL");
    *out = nullptr;
    rt_status st = stage_create("rt_exposure_create", device, 0, 0, out, [](rt_exposure &e) { return e.block.ensure(sizeof(ToneMapRequest::State)); });
    if (st == RT_OK && (st = exposure_clear(*out))) { stage_destroy(*out); *out = nullptr; }
    return st;
}

extern "C" rt_status rt_exposure_reset(rt_exposure *e)
{
    if (!e) return fail(RT_ERR_ARG, "rt_exposure_reset: state is NULL");
    HIP_TRY(hipSetDevice(e->device));
    std::lock_guard<std::mutex> lk(e->mu);
    return exposure_clear(e);
}

extern "C" void rt_exposure_destroy(rt_exposure *e) { stage_destroy(e); }

// waits for the calls issued on the state and copies its block to the host
static rt_status exposure_read(const char *name, rt_exposure *e, ToneMapRequest::State &out)
{
    if (!e) return fail(RT_ERR_ARG, "%s: state is NULL", name);
    HIP_TRY(hipSetDevice(e->device));
    std::lock_guard<std::mutex> lk(e->mu);
    rt_status rs = e->sync.wait_host();
    if (rs) return rs;
    HIP_TRY(hipMemcpy(&out, e->block.p, sizeof out, hipMemcpyDeviceToHost));
    return RT_OK;
}

extern "C" rt_status rt_exposure_get(rt_exposure *e, float *log2_exposure, double *log2_metered, uint32_t *metered_pixels)
{
    ToneMapRequest::State s;
    rt_status st = exposure_read("rt_exposure_get", e, s);
    if (st) return st;
    if (log2_exposure) *log2_exposure = s.E;
    if (log2_metered) *log2_metered = s.lbar;
    if (metered_pixels) *metered_pixels = s.n;
    return RT_OK;
}

extern "C" rt_status rt_exposure_histogram(rt_exposure *e, uint32_t out[256])
{
    if (!out) return fail(RT_ERR_ARG, "rt_exposure_histogram: out is NULL");
    ToneMapRequest::State s;
    rt_status st = exposure_read("rt_exposure_histogram", e, s);
    if (st) return st;
    memcpy(out, s.last, sizeof s.last);
    return RT_OK;
}

extern "C" void rt_tonemap_default_params(rt_tonemap_params *p)
{
    if (!p) return;
    p->struct_size = (uint32_t)sizeof *p;
    p->op = RT_TONEMAP_ACES; p->auto_exposure = 1;
    p->key = 0.18f; p->ev_bias = 0.0f; p->ev_min = -16.0f; p->ev_max = 16.0f; p->p_low = 0.10f; p->p_high = 0.90f;
    p->adapt_up = 1.0f; p->adapt_down = 1.0f; p->white = 4.0f; p->gamma = 2.2f;
}

// everything that can be refused before a launch, for both entry points: the device is looked for last
static rt_status tonemap_check(const char *name, const rt_exposure *e, int device, int32_t w, int32_t h, const rt_tonemap_params *p, const rt_tonemap_planes *pl)
{
    rt_status st = check_params_planes(name, "rt_tonemap_params", p, "rt_tonemap_planes", pl);
    if (st || (st = check_image_dims(name, w, h))) return st;
    if (p->op != RT_TONEMAP_CLAMP && p->op != RT_TONEMAP_REINHARD && p->op != RT_TONEMAP_ACES) return fail(RT_ERR_ARG, "%s: no operator %d", name, p->op);
    for (float s : {p->key, p->white, p->gamma})
        if (!(s > 0.0f) || !std::isfinite(s)) return fail(RT_ERR_ARG, "%s: key, white and gamma must be positive and finite", name);
    if (!std::isfinite(p->ev_bias) || !std::isfinite(p->ev_min) || !std::isfinite(p->ev_max) || !(p->ev_min <= p->ev_max))
        return fail(RT_ERR_ARG, "%s: ev_bias, ev_min and ev_max must be finite and ev_min <= ev_max", name);
    if (!(p->p_low >= 0.0f && p->p_low < p->p_high && p->p_high <= 1.0f)) return fail(RT_ERR_ARG, "%s: the percentiles must be 0 <= p_low < p_high <= 1", name);
    for (float a : {p->adapt_up, p->adapt_down})
        if (!(a > 0.0f && a <= 1.0f)) return fail(RT_ERR_ARG, "%s: adapt_up and adapt_down must be in (0, 1]", name);
    if (!pl->rgb_linear) return fail(RT_ERR_ARG, "%s: rgb_linear is required", name);
    if (!pl->out_display && !pl->out_rgb8) return fail(RT_ERR_ARG, "%s: one of out_display and out_rgb8 is required", name);
    if (p->auto_exposure && !e) return fail(RT_ERR_ARG, "%s: auto-exposure needs an rt_exposure", name);
    if (e && e->device != device) return fail(RT_ERR_ARG, "%s: the state is on device %d, the call names %d", name, e->device, device);
    if ((st = check_image_limit(name, w, h))) return st;
    return need_gfx950(name, device);
}

static rt_status tonemap_on_device(rt_exposure *e, int device, hipStream_t st, int32_t w, int32_t h, const rt_tonemap_params *p,
                                   const rt_tonemap_planes *pl, int sync)
{
    HIP_TRY(hipSetDevice(device));
    ToneMapRequest R = {};
    R.width = w; R.height = h; R.op = p->op; R.meter = p->auto_exposure != 0;
    R.log2_key = log2((double)p->key);
    R.ev_bias = p->ev_bias; R.ev_min = p->ev_min; R.ev_max = p->ev_max; R.p_low = p->p_low; R.p_high = p->p_high;
    R.adapt_up = p->adapt_up; R.adapt_down = p->adapt_down;
    R.scale = (float)exp2((double)p->ev_bias);
    R.white2 = (float)((double)p->white * (double)p->white);
    R.inv_gamma = display_inv_gamma(p->gamma);
    R.rgb_linear = pl->rgb_linear; R.object_id = pl->object_id; R.out_display = pl->out_display; R.out_rgb8 = pl->out_rgb8;
    if (!R.meter) {                     // fixed exposure: nothing of the state is read or written, nothing to order
        rtk_launch_tonemap(st, R);
        HIP_TRY(hipGetLastError());
        if (sync) HIP_TRY(hipStreamSynchronize(st));
        return RT_OK;
    }
    std::lock_guard<std::mutex> lk(e->mu);
    rt_status rs = e->sync.wait(st);
    if (rs) return rs;
    R.state = (ToneMapRequest::State *)e->block.p;
    rtk_launch_tonemap(st, R);
    HIP_TRY(hipGetLastError());
    return e->sync.settle(st, sync);
}

extern "C" rt_status rt_tonemap_device(rt_exposure *e, int device, void *hip_stream, int32_t w, int32_t h, const rt_tonemap_params *p,
                                       const rt_tonemap_planes *device_planes, int sync)
{
    rt_status st = tonemap_check("rt_tonemap_device", e, device, w, h, p, device_planes);
    return st ? st : tonemap_on_device(e, device, (hipStream_t)hip_stream, w, h, p, device_planes, sync);
}

extern "C" rt_status rt_tonemap(rt_exposure *e, int device, int32_t w, int32_t h, const rt_tonemap_params *p, const rt_tonemap_planes *host_planes)
{
    rt_status st = tonemap_check("rt_tonemap", e, device, w, h, p, host_planes);
    if (st) return st;
    HIP_TRY(hipSetDevice(device));
    const size_t n = (size_t)w * (size_t)h;
    HostPlanes S;                                                   // the display plane is written in place into the uploaded colour
    const int rgb = S.in(host_planes->rgb_linear, n * 12, host_planes->out_display), id = S.in(host_planes->object_id, n * 4);
    const int rgb8 = S.out(host_planes->out_rgb8, n * 3);
    if (S.st) return S.st;
    const rt_tonemap_planes dev = {(uint32_t)sizeof dev, S.dev<float>(rgb), S.dev<int32_t>(id), S.dev_out<float>(rgb), S.dev<uint8_t>(rgb8)};
    if ((st = tonemap_on_device(e, device, nullptr, w, h, p, &dev, 1))) return st;
    return S.download({rgb, rgb8});
}

// ---- bloom ------------------------------------------------------------------------------------------------------------------
// An rt_bloom owns the pyramid of one W x H stream of frames on its device -- every level the size allows, whatever `levels` a
// call asks for -- and the event that orders a call behind the previous one on the same object.
struct rt_bloom : StageObject { DevBuf pyramid; void release() { pyramid.release(); } };

extern "C" rt_status rt_bloom_create(int device, int32_t w, int32_t h, rt_bloom **out)
{
    if (!out) return fail(RT_ERR_ARG, "rt_bloom_create: out is NULL");
    *out = nullptr;
    rt_status st = check_image_size("rt_bloom_create", w, h);
    if (st) return st;
    return stage_create("rt_bloom_create", device, w, h, out, [](rt_bloom &b) {
        const BloomPlan all = rtk_bloom_plan(b.w, b.h, RT_BLOOM_MAX_LEVELS);
        return b.pyramid.ensure(all.off[all.levels] * 12);
    });
}

extern "C" void rt_bloom_destroy(rt_bloom *b) { stage_destroy(b); }

extern "C" void rt_bloom_default_params(rt_bloom_params *p)
{
    if (!p) return;
    p->struct_size = (uint32_t)sizeof *p;
    p->threshold = 1.0f; p->knee = 0.5f; p->intensity = 0.25f; p->spread = 0.7f; p->levels = 6; p->exposure_ev = 0.0f;
}

extern "C" rt_status rt_bloom_plan(int32_t w, int32_t h, int32_t levels, int32_t *levels_used, int32_t *tail_level)
{
    rt_status st = check_image_dims("rt_bloom_plan", w, h);
    if (st) return st;
    if (levels < 1) return fail(RT_ERR_ARG, "rt_bloom_plan: levels is %d, must be at least 1", levels);
    const BloomPlan P = rtk_bloom_plan(w, h, levels);
    if (levels_used) *levels_used = P.levels;
    if (tail_level) *tail_level = P.tail;
    return RT_OK;
}

// everything that can be refused without a device, for both entry points
static rt_status bloom_check(const char *name, const rt_bloom *b, const rt_exposure *e, const rt_bloom_params *p, const rt_bloom_planes *pl)
{
    rt_status st = check_params_planes(name, "rt_bloom_params", p, "rt_bloom_planes", pl);
    if (st) return st;
    for (float s : {p->threshold, p->knee, p->intensity, p->spread})
        if (!(s >= 0.0f) || !std::isfinite(s)) return fail(RT_ERR_ARG, "%s: threshold, knee, intensity and spread must be finite and not negative", name);
    if (p->spread > 1.0f || p->knee > 1.0f) return fail(RT_ERR_ARG, "%s: spread and knee must be at most 1", name);
    if (p->levels < 1) return fail(RT_ERR_ARG, "%s: levels is %d, must be at least 1", name, p->levels);
    if (!std::isfinite(p->exposure_ev)) return fail(RT_ERR_ARG, "%s: exposure_ev must be finite", name);
    if (!pl->rgb_linear) return fail(RT_ERR_ARG, "%s: rgb_linear is required", name);
    if (!pl->out && !pl->out_bloom) return fail(RT_ERR_ARG, "%s: one of out and out_bloom is required", name);
    // what needs the object comes last: without a device there is none, and everything above is still refused by name
    if (!b) return fail(RT_ERR_ARG, "%s: the rt_bloom is NULL", name);
    if (e && e->device != b->device) return fail(RT_ERR_ARG, "%s: the exposure state is on device %d, the rt_bloom on %d", name, e->device, b->device);
    const size_t bytes = (size_t)b->w * (size_t)b->h * 12;
    if ((pl->out != pl->rgb_linear && planes_overlap(pl->out, bytes, pl->rgb_linear, bytes)) || planes_overlap(pl->out_bloom, bytes, pl->rgb_linear, bytes) ||
        planes_overlap(pl->out_bloom, bytes, pl->out, bytes))
        return fail(RT_ERR_ARG, "%s: planes overlap (only out == rgb_linear is allowed)", name);
    return RT_OK;
}

static rt_status bloom_on_device(rt_bloom *b, rt_exposure *e, hipStream_t st, const rt_bloom_params *p, const rt_bloom_planes *pl, int sync)
{
    HIP_TRY(hipSetDevice(b->device));
    BloomRequest R = {};
    R.width = b->w; R.height = b->h;
    R.threshold = p->threshold; R.knee_k = p->knee * p->threshold; R.intensity = p->intensity;
    R.spread = p->spread; R.one_minus_spread = 1.0f - p->spread;
    R.scale = (float)exp2((double)p->exposure_ev);
    R.rgb_linear = pl->rgb_linear; R.out = pl->out; R.out_bloom = pl->out_bloom;
    R.plan = rtk_bloom_plan(b->w, b->h, p->levels);
    std::lock_guard<std::mutex> lk(b->mu);          // two objects: the bloom's mutex first, then the state's
    std::unique_lock<std::mutex> le;
    if (e) le = std::unique_lock<std::mutex>(e->mu);
    R.pyramid = (float *)b->pyramid.p;
    rt_status rs = b->sync.wait(st);
    if (rs) return rs;
    if (e) {                            // the state is read: behind the calls that write it, and the next one of them behind this
        if ((rs = e->sync.wait(st))) return rs;
        R.state = (const ToneMapRequest::State *)e->block.p;
    }
    HIP_TRY(rtk_launch_bloom(st, R));
    if ((rs = b->sync.record(st)) || (e && (rs = e->sync.record(st)))) return rs;
    if (sync) { HIP_TRY(hipStreamSynchronize(st)); b->sync.pending = false; if (e) e->sync.pending = false; }
    return RT_OK;
}

extern "C" rt_status rt_bloom_device(rt_bloom *b, rt_exposure *e, void *hip_stream, const rt_bloom_params *p,
                                     const rt_bloom_planes *device_planes, int sync)
{
    rt_status st = bloom_check("rt_bloom_device", b, e, p, device_planes);
    return st ? st : bloom_on_device(b, e, (hipStream_t)hip_stream, p, device_planes, sync);
}

extern "C" rt_status rt_bloom_host(rt_bloom *b, rt_exposure *e, const rt_bloom_params *p, const rt_bloom_planes *host_planes)
{
    rt_status st = bloom_check("rt_bloom_host", b, e, p, host_planes);
    if (st) return st;
    HIP_TRY(hipSetDevice(b->device));
    const size_t n = (size_t)b->w * (size_t)b->h;
    HostPlanes S;                                                   // `out` is written in place into the uploaded colour
    const int rgb = S.in(host_planes->rgb_linear, n * 12, host_planes->out), only = S.out(host_planes->out_bloom, n * 12);
    if (S.st) return S.st;
    const rt_bloom_planes dev = {(uint32_t)sizeof dev, S.dev<float>(rgb), S.dev_out<float>(rgb), S.dev<float>(only)};
    if ((st = bloom_on_device(b, e, nullptr, p, &dev, 1))) return st;
    return S.download({rgb, only});
}

// ---- the tile-gather stages: what motion blur and depth of field share ------------------------------------------------------
// Both cut the image into K x K tiles, K (max_blur, max_coc) in 2..32, and keep a tile-max and a neighbour-max plane.
#define RT_TILE_MIN_K 2
#define RT_TILE_MAX_K 32
static size_t stage_tiles(int32_t w, int32_t h, int32_t K, int32_t *tx, int32_t *ty)
{
    const int32_t x = (w + K - 1) / K, y = (h + K - 1) / K;
    if (tx) *tx = x;
    if (ty) *ty = y;
    return (size_t)x * (size_t)y;
}
namespace {
// the two tile planes of an object: sized for K = 2, the most tiles a call can ask for
struct TilePlanes {
    DevBuf tile_max, tile_nmax;
    rt_status ensure(int32_t w, int32_t h, size_t bytes_per_tile)
    {
        const size_t bytes = stage_tiles(w, h, RT_TILE_MIN_K, nullptr, nullptr) * bytes_per_tile;
        rt_status rs = tile_max.ensure(bytes);
        return rs ? rs : tile_nmax.ensure(bytes);
    }
    void release() { tile_max.release(); tile_nmax.release(); }
};
}
// `field`: what the stage calls its K
static rt_status check_tile_size(const char *name, const char *field, int32_t K)
{
    return K < RT_TILE_MIN_K || K > RT_TILE_MAX_K ? fail(RT_ERR_ARG, "%s: %s is %d, must be 2..32", name, field, K) : RT_OK;
}
static rt_status check_depth_extent(const char *name, float e)
{
    return !std::isfinite(e) || !(e >= 1e-3f) ? fail(RT_ERR_ARG, "%s: depth_extent must be finite and at least 1e-3", name) : RT_OK;
}
// no two of the (plane, bytes) that are given may share a byte; `why`: what the message says in brackets
#define RT_GATHER_READS_NEIGHBOURS "out may not be rgb_linear: the gather reads neighbours"
static rt_status check_planes_disjoint(const char *name, std::initializer_list<std::pair<const void *, size_t>> planes, const char *why)
{
    for (auto a = planes.begin(); a != planes.end(); a++)
        for (auto b = a + 1; b != planes.end(); b++)
            if (planes_overlap(a->first, a->second, b->first, b->second)) return fail(RT_ERR_ARG, "%s: planes overlap (%s)", name, why);
    return RT_OK;
}
// rt_motion_blur_tiles and rt_dof_tiles
static rt_status tiles_entry(const char *name, const char *field, int32_t w, int32_t h, int32_t K, int32_t *tx, int32_t *ty)
{
    rt_status st = check_image_dims(name, w, h);
    if (!st && !(st = check_tile_size(name, field, K))) stage_tiles(w, h, K, tx, ty);
    return st;
}
// the end of both _on_device functions: under the object's mutex the request's head, the wait, the launch and the record
template <class T, class R, class L> static rt_status tile_stage_run(T *o, hipStream_t st, int sync, int32_t K, int32_t N, R &req, L launch)
{
    std::lock_guard<std::mutex> lk(o->mu);
    req.width = o->w; req.height = o->h; req.K = K; req.N = N;
    stage_tiles(o->w, o->h, K, &req.tiles_x, &req.tiles_y);
    req.tile_max = (float *)o->tiles.tile_max.p; req.tile_nmax = (float *)o->tiles.tile_nmax.p;
    rt_status rs = o->sync.wait(st);
    if (rs) return rs;
    HIP_TRY(launch(st, req));
    return o->sync.settle(st, sync);
}

// ---- motion blur ------------------------------------------------------------------------------------------------------------
// An rt_motion_blur owns the tile planes of one W x H stream of frames on its device, a float2 per tile, and the event that
// orders a call behind the previous one on the same object.
struct rt_motion_blur : StageObject { TilePlanes tiles; void release() { tiles.release(); } };

extern "C" rt_status rt_motion_blur_create(int device, int32_t w, int32_t h, rt_motion_blur **out)
{
    if (!out) return fail(RT_ERR_ARG, "rt_motion_blur_create: out is NULL");
    *out = nullptr;
    rt_status st = check_image_size("rt_motion_blur_create", w, h);
    if (st) return st;
    return stage_create("rt_motion_blur_create", device, w, h, out, [](rt_motion_blur &mb) { return mb.tiles.ensure(mb.w, mb.h, 8); });
}

extern "C" void rt_motion_blur_destroy(rt_motion_blur *mb) { stage_destroy(mb); }

extern "C" void rt_motion_blur_default_params(rt_motion_blur_params *p)
{
    if (!p) return;
    p->struct_size = (uint32_t)sizeof *p;
    p->shutter = 0.5f; p->max_blur = 16; p->samples = 15; p->depth_extent = 0.05f;
}

extern "C" rt_status rt_motion_blur_tiles(int32_t w, int32_t h, int32_t max_blur, int32_t *tx, int32_t *ty)
{
    return tiles_entry("rt_motion_blur_tiles", "max_blur", w, h, max_blur, tx, ty);
}

// everything that can be refused without a device, for both entry points
static rt_status mblur_check(const char *name, const rt_motion_blur *mb, const rt_motion_blur_params *p, const rt_motion_blur_planes *pl)
{
    rt_status st = check_params_planes(name, "rt_motion_blur_params", p, "rt_motion_blur_planes", pl);
    if (st) return st;
    if (!std::isfinite(p->shutter) || !(p->shutter >= 0.0f) || p->shutter > 2.0f) return fail(RT_ERR_ARG, "%s: shutter must be finite and 0..2", name);
    if ((st = check_tile_size(name, "max_blur", p->max_blur))) return st;
    if (p->samples < 3 || p->samples > 63 || !(p->samples & 1)) return fail(RT_ERR_ARG, "%s: samples is %d, must be odd and 3..63", name, p->samples);
    if ((st = check_depth_extent(name, p->depth_extent))) return st;
    if (!pl->rgb_linear || !pl->motion || !pl->z || !pl->out) return fail(RT_ERR_ARG, "%s: rgb_linear, motion, z and out are required", name);
    // what needs the object comes last: without a device there is none, and everything above is still refused by name
    if (!mb) return fail(RT_ERR_ARG, "%s: the rt_motion_blur is NULL", name);
    const size_t n = (size_t)mb->w * (size_t)mb->h;
    return check_planes_disjoint(name, {{pl->rgb_linear, n * 12}, {pl->motion, n * 12}, {pl->z, n * 4}, {pl->out, n * 12},
                                        {pl->out_tiles, stage_tiles(mb->w, mb->h, p->max_blur, nullptr, nullptr) * 8}}, RT_GATHER_READS_NEIGHBOURS);
}

static rt_status mblur_on_device(rt_motion_blur *mb, hipStream_t st, const rt_motion_blur_params *p, const rt_motion_blur_planes *pl, int sync)
{
    HIP_TRY(hipSetDevice(mb->device));
    MotionBlurRequest R = {};
    R.half_shutter = 0.5f * p->shutter; R.two_over_n = 2.0f / (float)p->samples; R.depth_extent = p->depth_extent;
    R.rgb_linear = pl->rgb_linear; R.motion = pl->motion; R.z = pl->z; R.out = pl->out; R.out_tiles = pl->out_tiles;
    return tile_stage_run(mb, st, sync, p->max_blur, p->samples, R, rtk_launch_motion_blur);
}

extern "C" rt_status rt_motion_blur_device(rt_motion_blur *mb, void *hip_stream, const rt_motion_blur_params *p,
                                           const rt_motion_blur_planes *device_planes, int sync)
{
    rt_status st = mblur_check("rt_motion_blur_device", mb, p, device_planes);
    return st ? st : mblur_on_device(mb, (hipStream_t)hip_stream, p, device_planes, sync);
}

extern "C" rt_status rt_motion_blur_host(rt_motion_blur *mb, const rt_motion_blur_params *p, const rt_motion_blur_planes *host_planes)
{
    rt_status st = mblur_check("rt_motion_blur_host", mb, p, host_planes);
    if (st) return st;
    HIP_TRY(hipSetDevice(mb->device));
    const size_t n = (size_t)mb->w * (size_t)mb->h;
    const size_t tile_bytes = stage_tiles(mb->w, mb->h, p->max_blur, nullptr, nullptr) * 8;
    HostPlanes S;
    const int rgb = S.in(host_planes->rgb_linear, n * 12), motion = S.in(host_planes->motion, n * 12), z = S.in(host_planes->z, n * 4);
    const int out = S.out(host_planes->out, n * 12), tiles = S.out(host_planes->out_tiles, tile_bytes);
    if (S.st) return S.st;
    const rt_motion_blur_planes dev = {(uint32_t)sizeof dev, S.dev<float>(rgb), S.dev<float>(motion), S.dev<float>(z),
                                       S.dev<float>(out), S.dev<float>(tiles)};
    if ((st = mblur_on_device(mb, nullptr, p, &dev, 1))) return st;
    return S.download({out, tiles});
}

// ---- depth of field -------------------------------------------------------------------------------------------------------
// An rt_dof owns the (c, D) plane and the tile planes of one W x H stream of frames on its device, a float per tile, and the
// event that orders a call behind the previous one on the same object.
#define RT_DOF_MIN_N 8
#define RT_DOF_MAX_FOCUS 1e20f
struct rt_dof : StageObject { DevBuf coc; TilePlanes tiles; void release() { coc.release(); tiles.release(); } };

// step 5's table: a Vogel spiral in double, rounded to float once per coordinate
static void dof_tap_table(int32_t N, float *xy)
{
    const double golden = M_PI * (3.0 - sqrt(5.0));
    for (int32_t i = 0; i < N; i++) {
        const double rho = sqrt(((double)i + 0.5) / (double)N), phi = (double)i * golden;
        xy[2 * i] = (float)(rho * cos(phi)); xy[2 * i + 1] = (float)(rho * sin(phi));
    }
}

extern "C" rt_status rt_dof_create(int device, int32_t w, int32_t h, rt_dof **out)
{
    if (!out) return fail(RT_ERR_ARG, "rt_dof_create: out is NULL");
    *out = nullptr;
    rt_status st = check_image_size("rt_dof_create", w, h);
    if (st) return st;
    return stage_create("rt_dof_create", device, w, h, out, [](rt_dof &d) {
        rt_status rs = d.coc.ensure((size_t)d.w * (size_t)d.h * 8);
        return rs ? rs : d.tiles.ensure(d.w, d.h, 4);
    });
}

extern "C" void rt_dof_destroy(rt_dof *d) { stage_destroy(d); }

extern "C" void rt_dof_default_params(rt_dof_params *p)
{
    if (!p) return;
    p->struct_size = (uint32_t)sizeof *p;
    p->max_coc = 16; p->samples = 32; p->depth_extent = 0.05f; p->aperture_scale = 1.0f; p->focus = 0.0f;
}

extern "C" rt_status rt_dof_tiles(int32_t w, int32_t h, int32_t max_coc, int32_t *tx, int32_t *ty)
{
    return tiles_entry("rt_dof_tiles", "max_coc", w, h, max_coc, tx, ty);
}

extern "C" rt_status rt_dof_taps(int32_t samples, float *xy)
{
    if (!xy) return fail(RT_ERR_ARG, "rt_dof_taps: xy is NULL");
    if (samples < RT_DOF_MIN_N || samples > RT_DOF_MAX_TAPS) return fail(RT_ERR_ARG, "rt_dof_taps: samples is %d, must be 8..64", samples);
    dof_tap_table(samples, xy);
    return RT_OK;
}

// everything that can be refused without a device, for both entry points; on success *A and *fd are step 0's
static rt_status dof_check(const char *name, const rt_dof *d, const rt_camera *cam, const rt_dof_params *p, const rt_dof_planes *pl, float *A, float *fd)
{
    if (!cam) return fail(RT_ERR_ARG, "%s: the camera is NULL", name);
    rt_status st = check_params_planes(name, "rt_dof_params", p, "rt_dof_planes", pl);
    if (st) return st;
    if ((st = check_tile_size(name, "max_coc", p->max_coc))) return st;
    if (p->samples < RT_DOF_MIN_N || p->samples > RT_DOF_MAX_TAPS) return fail(RT_ERR_ARG, "%s: samples is %d, must be 8..64", name, p->samples);
    if ((st = check_depth_extent(name, p->depth_extent))) return st;
    if (!std::isfinite(p->aperture_scale) || !(p->aperture_scale >= 0.0f)) return fail(RT_ERR_ARG, "%s: aperture_scale must be finite and not negative", name);
    if (p->focus != 0.0f && !(p->focus > 0.0f && p->focus <= RT_DOF_MAX_FOCUS)) return fail(RT_ERR_ARG, "%s: focus must be 0 (the camera's focaldist) or in (0, 1e20]", name);
    if (!pl->rgb_linear || !pl->z || !pl->out) return fail(RT_ERR_ARG, "%s: rgb_linear, z and out are required", name);
    if (!(cam->fov > 0.0f && cam->fov < 180.0f)) return fail(RT_ERR_ARG, "%s: the camera's fov must be in (0, 180)", name);
    if (!std::isfinite(cam->dof)) return fail(RT_ERR_ARG, "%s: the camera's dof must be finite", name);
    *fd = p->focus != 0.0f ? p->focus : cam->focaldist;
    if (!(*fd > 0.0f && *fd <= RT_DOF_MAX_FOCUS)) return fail(RT_ERR_ARG, "%s: the camera's focaldist must be in (0, 1e20]", name);
    if ((st = check_image_dims(name, cam->width, cam->height))) return st;
    const double a = ((double)p->aperture_scale * fabs((double)cam->dof) * (double)cam->height) /
                     (2.0 * (double)*fd * tan((double)cam->fov / 2 * (M_PI / 180)));
    *A = (float)a;
    if (!std::isfinite(*A)) return fail(RT_ERR_ARG, "%s: the camera's aperture in pixels (A) is not finite", name);
    if ((st = check_image_limit(name, cam->width, cam->height))) return st;
    const size_t n = (size_t)cam->width * (size_t)cam->height;
    if ((st = check_planes_disjoint(name, {{pl->rgb_linear, n * 12}, {pl->z, n * 4}, {pl->out, n * 12}, {pl->out_coc, n * 4},
                                           {pl->out_tiles, stage_tiles(cam->width, cam->height, p->max_coc, nullptr, nullptr) * 4}}, RT_GATHER_READS_NEIGHBOURS)))
        return st;
    // what needs the object comes last: without a device there is none, and everything above is still refused by name
    if (!d) return fail(RT_ERR_ARG, "%s: the rt_dof is NULL", name);
    if (cam->width != d->w || cam->height != d->h)
        return fail(RT_ERR_ARG, "%s: the camera is %d x %d, the rt_dof %d x %d", name, cam->width, cam->height, d->w, d->h);
    return RT_OK;
}

static rt_status dof_on_device(rt_dof *d, hipStream_t st, const rt_camera *cam, float A, float fd, const rt_dof_params *p, const rt_dof_planes *pl, int sync)
{
    HIP_TRY(hipSetDevice(d->device));
    DofRequest R = {};
    R.A = A; R.focus = fd; R.depth_extent = p->depth_extent;
    DevCamera dc;
    camera_setup(*cam, dc);
    R.bx = dc.b[0]; R.by = dc.b[1]; R.u = dc.u; R.v = dc.v; R.l = -dc.b[2];
    float taps[2 * RT_DOF_MAX_TAPS];
    dof_tap_table(p->samples, taps);
    R.taps = taps;
    R.rgb_linear = pl->rgb_linear; R.z = pl->z; R.out = pl->out; R.out_coc = pl->out_coc; R.out_tiles = pl->out_tiles;
    R.coc = (float2 *)d->coc.p;                                 // (set once, by the create)
    return tile_stage_run(d, st, sync, p->max_coc, p->samples, R, rtk_launch_dof);
}

extern "C" rt_status rt_dof_device(rt_dof *d, void *hip_stream, const rt_camera *cam, const rt_dof_params *p, const rt_dof_planes *device_planes, int sync)
{
    float A, fd;
    rt_status st = dof_check("rt_dof_device", d, cam, p, device_planes, &A, &fd);
    return st ? st : dof_on_device(d, (hipStream_t)hip_stream, cam, A, fd, p, device_planes, sync);
}

extern "C" rt_status rt_dof_host(rt_dof *d, const rt_camera *cam, const rt_dof_params *p, const rt_dof_planes *host_planes)
{
    float A, fd;
    rt_status st = dof_check("rt_dof_host", d, cam, p, host_planes, &A, &fd);
    if (st) return st;
    HIP_TRY(hipSetDevice(d->device));
    const size_t n = (size_t)d->w * (size_t)d->h;
    const size_t tile_bytes = stage_tiles(d->w, d->h, p->max_coc, nullptr, nullptr) * 4;
    HostPlanes S;
    const int rgb = S.in(host_planes->rgb_linear, n * 12), z = S.in(host_planes->z, n * 4);
    const int out = S.out(host_planes->out, n * 12), coc = S.out(host_planes->out_coc, n * 4), tiles = S.out(host_planes->out_tiles, tile_bytes);
    if (S.st) return S.st;
    const rt_dof_planes dev = {(uint32_t)sizeof dev, S.dev<float>(rgb), S.dev<float>(z), S.dev<float>(out), S.dev<float>(coc), S.dev<float>(tiles)};
    if ((st = dof_on_device(d, nullptr, cam, A, fd, p, &dev, 1))) return st;
    return S.download({out, coc, tiles});
}
