// rt_shim.cpp -- BeginRender/StopRender/saveImage + RenderImage over the C ABI (see rt_shim.h).
#include "rt_shim.h"

#include <cstring>

namespace rt {

void RenderImage::Init(int w, int h)
{
    width = w; height = h;
    img.assign((size_t)w * h * 3, 0);
    zbuffer.assign((size_t)w * h, 0.0f);
    sampleCount.assign((size_t)w * h, 0);
    zbufferImg.clear(); sampleCountImg.clear();
    if (linearEnabled) linear.assign((size_t)w * h * 3, 0.0f);
    if (featuresEnabled) { featuresEnabled = false; EnableFeatures(); }
    if (varianceEnabled) variance.assign((size_t)w * h * 3, 0.0f);
    denoised.clear(); denoisedImg.clear(); denoisedVariance.clear();
    accumulated.clear(); accumulatedVariance.clear(); historyLength.clear(); motion.clear();
    rt_history_destroy(history);        // a history is of one size
    history = nullptr;
    display.clear(); displayImg.clear();
    rt_bloom_destroy(bloom);            // a pyramid is of one size
    bloom = nullptr;
    bloomed.clear();
    rt_motion_blur_destroy(motionBlur); // tile planes are of one size
    motionBlur = nullptr;
    motionBlurred.clear();
    rt_dof_destroy(dof);                // the (c, D) plane and the tile planes are of one size
    dof = nullptr;
    defocused.clear(); coc.clear();
    finalPixels = 0;
}

void RenderImage::EnableDepthOfField(const rt_dof_params *params)
{
    if (params) dofParams = *params;
    else rt_dof_default_params(&dofParams);
    dofEnabled = true;
}

void RenderImage::EnableMotionBlur(const rt_motion_blur_params *params)
{
    if (params) motionBlurParams = *params;
    else rt_motion_blur_default_params(&motionBlurParams);
    motionBlurEnabled = true;
}

void RenderImage::EnableBloom(const rt_bloom_params *params)
{
    if (params) bloomParams = *params;
    else rt_bloom_default_params(&bloomParams);
    bloomEnabled = true;
}

void RenderImage::ResetToneMap()
{
    if (exposure) rt_exposure_reset(exposure);
    display.clear(); displayImg.clear(); bloomed.clear(); motionBlurred.clear();
}

float RenderImage::ToneMapExposure() const
{
    float e = 0.0f;
    if (exposure) rt_exposure_get(exposure, &e, nullptr, nullptr);
    return e;
}

bool RenderImage::ToneMap(const rt_tonemap_params *params, int device)
{
    if (!toneMapEnabled || !linearEnabled) { toneMapError = "ToneMap() needs EnableToneMap() and EnableLinear() before the render"; return false; }
    if (!jobs.empty()) { toneMapError = "ToneMap() while the render is still running"; return false; }
    if (exposure && exposureDevice != device) { rt_exposure_destroy(exposure); exposure = nullptr; }
    if (!exposure && rt_exposure_create(device, &exposure) != RT_OK) { toneMapError = rt_last_error(); return false; }
    exposureDevice = device;
    rt_tonemap_params defaults;
    rt_tonemap_default_params(&defaults);
    const size_t n = (size_t)width * height;
    const std::vector<float> *from = !defocused.empty() ? &defocused : (!denoised.empty() ? &denoised : (!accumulated.empty() ? &accumulated : &linear));
    std::vector<float> smear;
    if (motionBlurEnabled && !motion.empty()) {     // along the motion plane of the last AccumulateTemporalMoving()
        if (motionBlur && motionBlurDevice != device) { rt_motion_blur_destroy(motionBlur); motionBlur = nullptr; }
        if (!motionBlur && rt_motion_blur_create(device, width, height, &motionBlur) != RT_OK) { toneMapError = rt_last_error(); return false; }
        motionBlurDevice = device;
        smear.resize(n * 3);
        const rt_motion_blur_planes mp = {(uint32_t)sizeof(rt_motion_blur_planes), from->data(), motion.data(), zbuffer.data(), smear.data(), nullptr};
        if (rt_motion_blur_host(motionBlur, &motionBlurParams, &mp) != RT_OK) { toneMapError = rt_last_error(); return false; }
        from = &smear;
    }
    std::vector<float> glare;
    if (bloomEnabled) {                 // ahead of the curve, relative to the scale the state holds from the call before
        if (bloom && bloomDevice != device) { rt_bloom_destroy(bloom); bloom = nullptr; }
        if (!bloom && rt_bloom_create(device, width, height, &bloom) != RT_OK) { toneMapError = rt_last_error(); return false; }
        bloomDevice = device;
        glare.resize(n * 3);
        const rt_bloom_planes bp = {(uint32_t)sizeof(rt_bloom_planes), from->data(), glare.data(), nullptr};
        if (rt_bloom_host(bloom, exposure, &bloomParams, &bp) != RT_OK) { toneMapError = rt_last_error(); return false; }
        from = &glare;
    }
    const std::vector<float> &src = *from;
    std::vector<float> out(n * 3);
    std::vector<uint8_t> out8(n * 3);
    const rt_tonemap_planes pl = {(uint32_t)sizeof(rt_tonemap_planes), src.data(), featuresEnabled ? objectIds.data() : nullptr, out.data(), out8.data()};
    if (rt_tonemap(exposure, device, width, height, params ? params : &defaults, &pl) != RT_OK) { toneMapError = rt_last_error(); return false; }
    display.swap(out); displayImg.swap(out8);
    if (bloomEnabled) bloomed.swap(glare);
    motionBlurred.swap(smear);          // empty again when the stage did not run
    toneMapError.clear();
    return true;
}

static rt_camera LowerCamera(const Camera &c);

// the lens over the most processed linear plane the image holds, from the z-buffer
bool RenderImage::DepthOfField(const Camera &c, int device)
{
    defocused.clear(); coc.clear();
    if (!dofEnabled || !linearEnabled) { dofError = "DepthOfField() needs EnableDepthOfField() and EnableLinear() before the render"; return false; }
    if (!jobs.empty()) { dofError = "DepthOfField() while the render is still running"; return false; }
    if (dof && dofDevice != device) { rt_dof_destroy(dof); dof = nullptr; }
    if (!dof && rt_dof_create(device, width, height, &dof) != RT_OK) { dofError = rt_last_error(); return false; }
    dofDevice = device;
    rt_camera rc = LowerCamera(c);
    rc.width = width; rc.height = height;
    const size_t n = (size_t)width * height;
    const std::vector<float> &from = !denoised.empty() ? denoised : (!accumulated.empty() ? accumulated : linear);
    std::vector<float> out(n * 3), radius(n);
    const rt_dof_planes pl = {(uint32_t)sizeof(rt_dof_planes), from.data(), zbuffer.data(), out.data(), radius.data(), nullptr};
    if (rt_dof_host(dof, &rc, &dofParams, &pl) != RT_OK) { dofError = rt_last_error(); return false; }
    defocused.swap(out); coc.swap(radius);
    dofError.clear();
    return true;
}

void RenderImage::ResetTemporal()
{
    if (history) rt_history_reset(history);
    accumulated.clear(); accumulatedVariance.clear(); historyLength.clear(); motion.clear(); clipped.clear();
}

void RenderImage::EnableTemporalClip(const rt_temporal_clip *clip)
{
    if (clip) temporalClip = *clip;
    else rt_temporal_clip_default(&temporalClip);
    temporalClipEnabled = true;
}

static rt_camera LowerCamera(const Camera &c)       // as Lower() hands the camera to the render
{
    rt_camera rc;
    rc.pos[0] = c.pos.x; rc.pos[1] = c.pos.y; rc.pos[2] = c.pos.z;
    rc.dir[0] = c.dir.x; rc.dir[1] = c.dir.y; rc.dir[2] = c.dir.z;
    rc.up[0] = c.up.x; rc.up[1] = c.up.y; rc.up[2] = c.up.z;
    rc.fov = c.fov; rc.focaldist = c.focaldist; rc.dof = c.dof; rc.width = c.imgWidth; rc.height = c.imgHeight;
    return rc;
}

bool RenderImage::AccumulateTemporal(const Camera &c, const rt_temporal_params *params, int device)
{
    return Accumulate(c, nullptr, nullptr, nullptr, 0, params, device);
}

bool RenderImage::AccumulateTemporalMoving(const Camera &c, const Camera &prev, const rt_node *nodes, const rt_node *prevNodes, int n,
                                           const rt_temporal_params *params, int device)
{
    return Accumulate(c, &prev, nodes, prevNodes, n, params, device);
}

// prev == NULL: rt_temporal; otherwise rt_motion of this frame first, then rt_temporal_motion with its plane.  After
// EnableTemporalClip(): rt_temporal_clip_host in place of both, with or without the plane
bool RenderImage::Accumulate(const Camera &c, const Camera *prev, const rt_node *nodes, const rt_node *prevNodes, int nNodes,
                             const rt_temporal_params *params, int device)
{
    if (!temporalEnabled || !linearEnabled || !featuresEnabled) {
        temporalError = "AccumulateTemporal() needs EnableTemporal(), EnableLinear() and EnableFeatures() before the render";
        return false;
    }
    if (!jobs.empty()) { temporalError = "AccumulateTemporal() while the render is still running"; return false; }
    if (history && historyDevice != device) { rt_history_destroy(history); history = nullptr; }
    if (!history && rt_history_create(device, width, height, &history) != RT_OK) { temporalError = rt_last_error(); return false; }
    historyDevice = device;
    const rt_camera rc = LowerCamera(c);
    rt_temporal_params defaults;
    rt_temporal_default_params(&defaults);
    const size_t n = (size_t)width * height;
    std::vector<float> out(n * 3), outVar(varianceEnabled ? n * 3 : 0), len(n);
    const rt_temporal_planes pl = {(uint32_t)sizeof(rt_temporal_planes), linear.data(), normals.data(), albedo.data(), zbuffer.data(),
                                   objectIds.data(), varianceEnabled ? variance.data() : nullptr, out.data(),
                                   varianceEnabled ? outVar.data() : nullptr, len.data(), nullptr};
    std::vector<float> mask(temporalClipEnabled ? n : 0);
    rt_temporal_clip clip = temporalClip;
    clip.out_clipped = mask.data();
    if (prev) {
        const rt_camera prc = LowerCamera(*prev);
        std::vector<float> mv(n * 3);
        const rt_motion_planes mp = {(uint32_t)sizeof(rt_motion_planes), zbuffer.data(), objectIds.data(), mv.data()};
        if (rt_motion(device, &rc, &prc, nodes, prevNodes, nNodes, &mp) != RT_OK ||
            (temporalClipEnabled ? rt_temporal_clip_host(history, &rc, params ? params : &defaults, &clip, &pl, mv.data())
                                 : rt_temporal_motion(history, &rc, params ? params : &defaults, &pl, mv.data())) != RT_OK) { temporalError = rt_last_error(); return false; }
        motion.swap(mv);
    } else {
        if ((temporalClipEnabled ? rt_temporal_clip_host(history, &rc, params ? params : &defaults, &clip, &pl, nullptr)
                                 : rt_temporal(history, &rc, params ? params : &defaults, &pl)) != RT_OK) { temporalError = rt_last_error(); return false; }
        motion.clear();
    }
    clipped.swap(mask);
    defocused.clear(); coc.clear();     // of the plane before this one
    accumulated.swap(out); accumulatedVariance.swap(outVar); historyLength.swap(len);
    temporalError.clear();
    return true;
}

void RenderImage::EnableVariance()
{
    if (!varianceEnabled) variance.assign((size_t)width * height * 3, 0.0f);
    varianceEnabled = true;
}

void RenderImage::EnableFeatures()
{
    if (!featuresEnabled) {
        const size_t n = (size_t)width * height;
        normals.assign(n * 3, 0.0f); albedo.assign(n * 3, 0.0f); alpha.assign(n, 0.0f); objectIds.assign(n, -1);
    }
    featuresEnabled = true;
}

// a multiplicative hash of id + 1, so that neighbouring ids get unrelated colours; every channel at least 64: no object is black
void RenderImage::ObjectIdColor(int32_t id, uint8_t rgb[3])
{
    if (id < 0) { rgb[0] = rgb[1] = rgb[2] = 0; return; }
    const uint32_t h = ((uint32_t)id + 1u) * 2654435761u;
    rgb[0] = (uint8_t)(64u + ((h >> 8) & 0xFFu) % 192u); rgb[1] = (uint8_t)(64u + ((h >> 16) & 0xFFu) % 192u); rgb[2] = (uint8_t)(64u + ((h >> 24) & 0xFFu) % 192u);
}

bool RenderImage::SaveFeatureImages(const char *prefix) const
{
    if (!featuresEnabled || !prefix) return false;
    const std::string p(prefix);
    std::vector<uint8_t> ids(objectIds.size() * 3);
    for (size_t i = 0; i < objectIds.size(); i++) ObjectIdColor(objectIds[i], &ids[3 * i]);
    return WritePFM((p + "_normal.pfm").c_str(), normals.data(), width, height) && WritePFM((p + "_albedo.pfm").c_str(), albedo.data(), width, height) &&
           WritePFM((p + "_alpha.pfm").c_str(), alpha.data(), width, height, 1) && WritePNG((p + "_id.png").c_str(), ids.data(), width, height, 3);
}

void RenderImage::EnableLinear()
{
    if (!linearEnabled) linear.assign((size_t)width * height * 3, 0.0f);
    linearEnabled = true;
}

bool RenderImage::DenoiseGuided(const rt_denoise_params *params, float k_sigma, int device)
{
    denoised.clear(); denoisedImg.clear(); denoisedVariance.clear(); defocused.clear(); coc.clear();
    if (!linearEnabled || !featuresEnabled || !varianceEnabled) {
        denoiseError = "DenoiseGuided() needs EnableLinear(), EnableFeatures() and EnableVariance() before the render";
        return false;
    }
    if (!jobs.empty()) { denoiseError = "DenoiseGuided() while the render is still running"; return false; }
    rt_denoise_params defaults;
    rt_denoise_default_params(&defaults);
    std::vector<float> out((size_t)width * height * 3), outVar((size_t)width * height * 3);
    std::vector<uint8_t> out8((size_t)width * height * 3);
    const rt_denoise_planes pl = {(uint32_t)sizeof(rt_denoise_planes), linear.data(), normals.data(), albedo.data(), zbuffer.data(),
                                  objectIds.data(), out.data(), out8.data()};
    rt_denoise_var v;
    rt_denoise_var_default(&v);
    v.variance = variance.data(); v.out_variance = outVar.data(); v.k_sigma = k_sigma;
    if (rt_denoise_var_host(device, width, height, params ? params : &defaults, &pl, &v) != RT_OK) { denoiseError = rt_last_error(); return false; }
    denoised.swap(out); denoisedImg.swap(out8); denoisedVariance.swap(outVar);
    denoiseError.clear();
    return true;
}

bool RenderImage::Denoise(const rt_denoise_params *params, int device)
{
    denoised.clear(); denoisedImg.clear(); denoisedVariance.clear(); defocused.clear(); coc.clear();
    if (!linearEnabled || !featuresEnabled) { denoiseError = "Denoise() needs EnableLinear() and EnableFeatures() before the render"; return false; }
    if (!jobs.empty()) { denoiseError = "Denoise() while the render is still running"; return false; }
    rt_denoise_params defaults;
    rt_denoise_default_params(&defaults);
    std::vector<float> out((size_t)width * height * 3);
    std::vector<uint8_t> out8((size_t)width * height * 3);
    const rt_denoise_planes pl = {(uint32_t)sizeof(rt_denoise_planes), linear.data(), normals.data(), albedo.data(), zbuffer.data(),
                                  objectIds.data(), out.data(), out8.data()};
    if (rt_denoise(device, width, height, params ? params : &defaults, &pl) != RT_OK) { denoiseError = rt_last_error(); return false; }
    denoised.swap(out); denoisedImg.swap(out8);
    denoiseError.clear();
    return true;
}

int RenderImage::GetNumRenderedPixels() const
{
    if (jobs.empty()) return finalPixels;
    int n = 0;
    for (rt_job *j : jobs) n += rt_render_progress(j);
    return n;
}

// RenderImage::ComputeZBufferImage / ComputeSampleCountImage, FIN/include/scene.h:591-637 (rt_image.cpp)
void RenderImage::ComputeZBufferImage()
{
    zbufferImg.assign((size_t)width * height, 0);
    ZBufferImage(zbuffer.data(), zbufferImg.size(), zbufferImg.data());
}

int RenderImage::ComputeSampleCountImage()
{
    sampleCountImg.assign((size_t)width * height, 0);
    return SampleCountImage(sampleCount.data(), sampleCountImg.size(), sampleCountImg.data());
}

Renderer::Renderer() { rt_params_default(&params); rt_scene_create(&handle); }

Renderer::~Renderer()
{
    for (rt_job *j : jobs) { rt_render_stop(j); rt_render_wait(j); }
    renderImage.DetachJobs(0);
    for (rt_job *j : jobs) rt_job_destroy(j);
    rt_scene_destroy(handle);
}

int Renderer::LoadScene(const char *filename)
{
    lowered = false;
    if (!rt::LoadScene(scene, filename, &error)) return 0;
    renderImage.Init(scene.camera.imgWidth, scene.camera.imgHeight);
    return 1;
}

bool Renderer::SetPhotonMap(const rt_photon *balanced, uint32_t n_stored)
{
    if (rt_scene_set_photons(handle, balanced, n_stored) != RT_OK) { error = rt_last_error(); return false; }
    return true;
}

bool Renderer::BeginRender()
{
    if (!jobs.empty()) { error = "a render is already running"; return false; }
    SceneData d;
    if (!Lower(scene, d, &error)) return false;
    rt_status st = rt_scene_set_nodes(handle, d.nodes.data(), (int32_t)d.nodes.size());
    for (size_t m = 0; st == RT_OK && m < d.meshes.size(); m++) {
        const MeshData &md = d.meshes[m];
        st = rt_scene_set_mesh(handle, (int32_t)m, md.v.data(), (int32_t)(md.v.size() / 3), md.f.data(), (int32_t)(md.f.size() / 3),
                               md.vn.data(), (int32_t)(md.vn.size() / 3), md.fn.data(), md.nodes.data(), (int32_t)md.nodes.size(),
                               md.elements.data());
        if (st == RT_OK && !md.vt.empty())
            st = rt_scene_set_mesh_texcoords(handle, (int32_t)m, md.vt.data(), (int32_t)(md.vt.size() / 3), md.ft.data());
    }
    if (st == RT_OK) st = rt_scene_set_materials(handle, d.materials.data(), (int32_t)d.materials.size());
    if (st == RT_OK) st = rt_scene_set_lights(handle, d.lights.data(), (int32_t)d.lights.size());
    if (st == RT_OK) st = rt_scene_set_environment(handle, d.env, d.bg);
    if (st == RT_OK) st = rt_scene_set_textures(handle, d.textures.data(), (int32_t)d.textures.size(), d.texels.data(), (uint64_t)d.texels.size());
    if (st == RT_OK) st = rt_scene_set_material_maps(handle, d.material_maps.data(), d.material_maps.empty() ? 0 : (int32_t)d.materials.size());
    if (st == RT_OK) st = rt_scene_set_environment_maps(handle, &d.env_map, &d.bg_map);
    if (st != RT_OK) { error = rt_last_error(); return false; }
    if (renderImage.GetWidth() != d.camera.width || renderImage.GetHeight() != d.camera.height)
        renderImage.Init(d.camera.width, d.camera.height);
    if (st == RT_OK) st = rt_scene_set_photon_dump(handle, photonDump.empty() ? nullptr : photonDump.c_str());
    if (st == RT_OK) st = rt_scene_set_render_flags(handle, renderFlags);
    if (st != RT_OK) { error = rt_last_error(); return false; }
    // one job per device: device r of N renders the interleaved tiles r, r+N, ... into the SAME caller-owned buffers (a job
    // writes only the pixels of its own tiles); whichever job comes first runs the photon pass, the others wait for it
    std::vector<int> devs = devices;
    if (devs.empty()) for (int i = 0, n = rt_device_count(); i < n; i++) devs.push_back(i);
    if (devs.empty()) devs.push_back(0);              // no gfx950 device: rt_render_begin reports it (there is no CPU path)
    // the optional planes are NULL unless EnableLinear() / EnableFeatures(); EnableVariance() selects the _var entry point
    const rt_outputs o = {(uint32_t)sizeof(rt_outputs), renderImage.GetPixels(), renderImage.GetZBuffer(), renderImage.GetSampleCount(),
                          renderImage.GetLinearPixels(), renderImage.GetNormals(), renderImage.GetAlbedo(), renderImage.GetAlpha(),
                          renderImage.GetObjectIds()};
    const int N = (int)devs.size();
    for (int r = 0; r < N; r++) {
        const rt_tile_range mine = {32, 8, r, N};
        rt_job *job = nullptr;
        st = renderImage.GetVariance() ? rt_render_begin_outputs_var(handle, &d.camera, &params, &mine, devs[r], &o, renderImage.GetVariance(), &job)
                                       : rt_render_begin_outputs(handle, &d.camera, &params, &mine, devs[r], &o, &job);
        if (st != RT_OK) {
            error = rt_last_error();
            for (rt_job *j : jobs) { rt_render_stop(j); rt_render_wait(j); }
            renderImage.DetachJobs(0);
            for (rt_job *j : jobs) rt_job_destroy(j);
            jobs.clear();
            return false;
        }
        jobs.push_back(job);
        renderImage.AttachJob(job);
    }
    return true;
}

void Renderer::StopRender() { for (rt_job *j : jobs) rt_render_stop(j); }

bool Renderer::WaitRender()
{
    if (jobs.empty()) return true;
    bool ok = true;
    int pixels = 0;
    memset(&stats, 0, sizeof stats);
    memset(&setup, 0, sizeof setup);
    for (rt_job *j : jobs) {
        const rt_status st = rt_render_wait(j);
        if (st != RT_OK) { error = rt_last_error(); ok = false; }
        rt_stats one;
        if (rt_job_stats(j, &one) == RT_OK) {
            stats.rays_primary += one.rays_primary; stats.rays_shadow += one.rays_shadow; stats.rays_reflect += one.rays_reflect;
            stats.rays_refract += one.rays_refract; stats.photon_queries += one.photon_queries; stats.photons_visited += one.photons_visited;
            stats.pixels += one.pixels; stats.samples += one.samples;
            if (one.ms_total > stats.ms_total) stats.ms_total = one.ms_total;
        }
        rt_setup_ms su;
        if (rt_job_setup_ms(j, &su) == RT_OK && su.total > 0) setup = su;
        pixels += rt_render_progress(j);
    }
    renderImage.DetachJobs(pixels);
    for (rt_job *j : jobs) rt_job_destroy(j);
    jobs.clear();
    return ok;
}

// saveImage(), FIN/main.cpp:1000-1007
void Renderer::saveImage(const char *image, const char *samples, const char *zimage)
{
    renderImage.ComputeZBufferImage();
    if (zimage) renderImage.SaveZImage(zimage);
    if (image) renderImage.SaveImage(image);
    renderImage.ComputeSampleCountImage();
    if (samples) renderImage.SaveSampleCountImage(samples);
}

}  // namespace rt
