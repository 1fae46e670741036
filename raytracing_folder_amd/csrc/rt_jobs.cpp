// rt_jobs.cpp -- the asynchronous jobs of the C ABI in include/rt_mi355x.h: the rt_render_begin* entry points, whose worker thread
// runs the photon pass where one is due and then render_tiles (rt_render.cpp), and progress / stop / wait / statistics / destroy.
// struct rt_job itself is in rt_host.h (the orchestration reads and writes it); rt_host.h is what the host files share.
#include <mutex>
#include <string>
#include <thread>

#include "rt_host.h"

// BeginRender (FIN/main.cpp:984-1010): rt_render_begin, rt_render_begin_linear and rt_render_begin_outputs, with the planes
// RenderPixel (:273-338) could have kept: its colour before gamma, and the first hit's normal, albedo, coverage and node
static rt_status render_begin(const char *name, rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles, int device,
                              const rt_outputs *host_planes, rt_job **out, float *variance = nullptr)
{
    if (!s || !out) return fail(RT_ERR_ARG, "%s: scene/out is NULL", name);
    rt_status st = check_outputs(name, host_planes);
    if (st) return st;
    if ((st = validate_render(s, cam, p, tiles))) return st;
    DeviceState *D = nullptr;
    if ((st = prepare_device(s, device, &D))) return st;      // fail early (and loudly) when there is no GPU
    rt_job *job = new rt_job;
    job->scene = s;
    job->host = Planes(*host_planes, variance);
    s->live_jobs.fetch_add(1);
    const rt_camera camv = *cam; const rt_params pv = *p; const rt_tile_range tv = *tiles;
    job->worker = std::thread([=]() {
        auto body = [&]() -> rt_status {
            HIP_TRY(hipSetDevice(device));
            // BeginRender calls generatePhotonMap() before it spawns its workers (FIN/main.cpp:984-998, :350-402); here the
            // photon pass runs on the job's thread, so the call itself still returns at once and progress stays 0 meanwhile
            if (pv.shade_model == RT_SHADE_FIN && pv.photon_count > 0) {
                std::lock_guard<std::mutex> gen(s->gen_mu);         // one job per device may have been started: the first one generates
                bool have_map, have_source = false;
                std::string dump;
                {
                    std::lock_guard<std::mutex> lk(s->mu);
                    // a generated map serves only the parameters it was generated with (rt_photon_map.h)
                    have_map = s->global_photons.serves((uint32_t)pv.photon_count, pv.photon_bounce, pv.seed);
                    dump = s->photon_dump;
                }
                for (const rt_light &l : s->data.lights) if (l.type == RT_LIGHT_POINT) have_source = true;
                if (!have_map && have_source && !job->stop.load()) {
                    const rt_status g = generate_photons(s, device, (uint32_t)pv.photon_count, pv.photon_bounce, pv.seed, dump.empty() ? nullptr : dump.c_str(),
                                                         &job->setup, true);
                    if (g) return g;
                }
            }
            // a device copy of every plane that was asked for, starting from the caller's values -- but a strided job takes its
            // linear plane in its packed records and its features and variance in walk-indexed staging planes
            // (RenderAttempt::setup_outputs)
            RenderRequest req;
            req.job = job;
            req.rec_bytes = job->host.p[PL_LINEAR] ? 24 : 8;
            ScopedDevBuf dev[N_PLANES];
            const size_t npx = (size_t)camv.width * camv.height;
            for (int i = 0; i < N_PLANES; i++) {
                if (!job->host.p[i] || (tv.stride != 1 && i >= PL_LINEAR)) continue;
                if (rt_status us = dev[i].upload(job->host.p[i], npx * PLANE_BYTES[i])) return us;
                req.dev.p[i] = dev[i].p;
            }
            // render_tiles copies every finished band of rows back into the caller's buffers
            return render_tiles(s, &camv, &pv, &tv, device, req);
        };
        const rt_status r = body();
        job->status = r;
        if (r) job->error = rt_last_error();
        job->done.store(true);
        s->live_jobs.fetch_sub(1);
    });
    *out = job;
    return RT_OK;
}

extern "C" rt_status rt_render_begin(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles, int device,
                                     uint8_t *rgb8, float *z, uint8_t *count, rt_job **out)
{
    const rt_outputs o = outputs_of(rgb8, z, count);
    return render_begin("rt_render_begin", s, cam, p, tiles, device, &o, out);
}

extern "C" rt_status rt_render_begin_linear(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles, int device,
                                            uint8_t *rgb8, float *z, uint8_t *count, float *rgb_linear, rt_job **out)
{
    if (!rgb_linear) return fail(RT_ERR_ARG, "rt_render_begin_linear: the linear plane is required");
    const rt_outputs o = outputs_of(rgb8, z, count, rgb_linear);
    return render_begin("rt_render_begin_linear", s, cam, p, tiles, device, &o, out);
}

extern "C" rt_status rt_render_begin_outputs(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles, int device,
                                             const rt_outputs *host_planes, rt_job **out)
{
    return render_begin("rt_render_begin_outputs", s, cam, p, tiles, device, host_planes, out);
}

extern "C" rt_status rt_render_begin_outputs_var(rt_scene *s, const rt_camera *cam, const rt_params *p, const rt_tile_range *tiles, int device,
                                                 const rt_outputs *host_planes, float *variance, rt_job **out)
{
    if (!variance) return fail(RT_ERR_ARG, "rt_render_begin_outputs_var: the variance plane is required");
    return render_begin("rt_render_begin_outputs_var", s, cam, p, tiles, device, host_planes, out, variance);
}

extern "C" int rt_render_progress(rt_job *j) { return j ? j->progress.load() : 0; }
extern "C" rt_status rt_render_stop(rt_job *j) { if (!j) return fail(RT_ERR_ARG, "rt_render_stop: job is NULL"); j->stop.store(true); return RT_OK; }
extern "C" rt_status rt_render_wait(rt_job *j)
{
    if (!j) return fail(RT_ERR_ARG, "rt_render_wait: job is NULL");
    if (j->worker.joinable()) j->worker.join();
    if (j->status) return fail(j->status, "%s", j->error.c_str());      // the worker's message, on the waiting thread
    return j->status;
}
extern "C" rt_status rt_job_stats(rt_job *j, rt_stats *out)
{
    if (!j || !out) return fail(RT_ERR_ARG, "rt_job_stats: NULL argument");
    if (!j->done.load()) return fail(RT_ERR_STATE, "rt_job_stats: job still running");
    *out = j->stats;
    return RT_OK;
}
extern "C" rt_status rt_job_setup_ms(rt_job *j, rt_setup_ms *out)
{
    if (!j || !out) return fail(RT_ERR_ARG, "rt_job_setup_ms: NULL argument");
    if (!j->done.load()) return fail(RT_ERR_STATE, "rt_job_setup_ms: job still running");
    *out = j->setup;
    return RT_OK;
}
extern "C" void rt_job_destroy(rt_job *j)
{
    if (!j) return;
    j->stop.store(true);
    if (j->worker.joinable()) j->worker.join();
    delete j;
}
