// rt_shim.h -- the reference's driver surface on top of the C ABI.
//
// The reference's UI calls three free functions -- BeginRender() (must return immediately, the
// render proceeds in the background), StopRender() and saveImage() (FIN/viewport.cpp:35-37,
// 443-453) -- and polls renderImage.IsRenderDone() / reads renderImage.GetPixels() while the
// render runs (FIN/viewport.cpp:367,390-409).  rt::Renderer keeps exactly that contract:
// same method names and meaning, same RenderImage container (FIN/include/scene.h:540-656),
// but the pixels come from the HIP kernels through rt_render_begin().
#ifndef RT_HOST_SHIM_H
#define RT_HOST_SHIM_H

#include <string>
#include <vector>

#include "rt_scene.h"

namespace rt {

class RenderImage {
    std::vector<uint8_t> img;          // Color24[width*height]
    std::vector<float> zbuffer;
    std::vector<uint8_t> zbufferImg, sampleCount, sampleCountImg;
    std::vector<float> linear;         // opt-in (EnableLinear): pre-gamma float RGB[width*height*3]
    bool linearEnabled = false;
    // opt-in (EnableFeatures): the first-hit planes of rt_outputs -- normal, albedo (float RGB), alpha (float), object id
    std::vector<float> normals, albedo, alpha;
    std::vector<int32_t> objectIds;
    bool featuresEnabled = false;
    // Denoise(): the a-trous filter's outputs -- linear float RGB and its gamma-encoded Color24 image
    std::vector<float> denoised;
    std::vector<uint8_t> denoisedImg;
    // opt-in (EnableVariance): the variance plane of rt_render_begin_outputs_var (variance of the mean, float RGB); after a
    // DenoiseGuided() denoisedVariance holds the filtered one
    std::vector<float> variance, denoisedVariance;
    bool varianceEnabled = false;
    std::string denoiseError;
    // opt-in (EnableTemporal): the frames accumulated by AccumulateTemporal() -- linear float RGB, its variance (with
    // EnableVariance) and the per-pixel history length -- and the rt_history that holds them on the device
    std::vector<float> accumulated, accumulatedVariance, historyLength;
    std::vector<float> motion;         // AccumulateTemporalMoving(): the frame's motion plane, (fx, fy, z_exp) per pixel
    std::vector<float> clipped;        // EnableTemporalClip(): the rectification's mask of the last accumulated frame
    bool temporalEnabled = false, temporalClipEnabled = false;
    rt_temporal_clip temporalClip = {};
    rt_history *history = nullptr;
    int historyDevice = 0;
    std::string temporalError;
    // opt-in (EnableToneMap): ToneMap()'s outputs -- the display-referred float RGB and its gamma-encoded Color24 image -- and
    // the rt_exposure that carries the exposure from frame to frame on the device
    std::vector<float> display;
    std::vector<uint8_t> displayImg;
    bool toneMapEnabled = false;
    rt_exposure *exposure = nullptr;
    int exposureDevice = 0;
    std::string toneMapError;
    // opt-in (EnableBloom): ToneMap() blooms the plane first; the bloomed linear plane and the rt_bloom that owns the pyramid
    std::vector<float> bloomed;
    bool bloomEnabled = false;
    rt_bloom_params bloomParams = {};
    rt_bloom *bloom = nullptr;
    int bloomDevice = 0;
    // opt-in (EnableMotionBlur): ToneMap() blurs the plane along the last AccumulateTemporalMoving()'s motion plane first
    std::vector<float> motionBlurred;
    bool motionBlurEnabled = false;
    rt_motion_blur_params motionBlurParams = {};
    rt_motion_blur *motionBlur = nullptr;
    int motionBlurDevice = 0;
    // opt-in (EnableDepthOfField): DepthOfField()'s outputs -- the defocused linear plane and the signed circle of confusion per
    // pixel -- and the rt_dof that owns the stage's device planes
    std::vector<float> defocused, coc;
    bool dofEnabled = false;
    rt_dof_params dofParams = {};
    rt_dof *dof = nullptr;
    int dofDevice = 0;
    std::string dofError;
    int width = 0, height = 0;
    std::vector<rt_job *> jobs;        // progress sources while a render is live (one job per device)
    int finalPixels = 0;
    bool Accumulate(const Camera &camera, const Camera *prev, const rt_node *nodes, const rt_node *prevNodes, int nNodes,
                    const rt_temporal_params *params, int device);
public:
    RenderImage() = default;
    RenderImage(const RenderImage &) = delete;
    RenderImage &operator=(const RenderImage &) = delete;
    ~RenderImage() { rt_history_destroy(history); rt_dof_destroy(dof); rt_motion_blur_destroy(motionBlur); rt_bloom_destroy(bloom); rt_exposure_destroy(exposure); }
    void Init(int w, int h);
    int GetWidth() const { return width; }
    int GetHeight() const { return height; }
    uint8_t *GetPixels() { return img.data(); }
    float *GetZBuffer() { return zbuffer.data(); }
    uint8_t *GetZBufferImage() { return zbufferImg.data(); }
    uint8_t *GetSampleCount() { return sampleCount.data(); }
    uint8_t *GetSampleCountImage() { return sampleCountImg.data(); }
    // the linear (pre-gamma) float RGB plane, row-major like GetPixels(); nothing is allocated until EnableLinear(), and
    // GetLinearPixels() is NULL without it.  Renderer::BeginRender fills it through rt_render_begin_outputs.
    void EnableLinear();
    bool LinearEnabled() const { return linearEnabled; }
    float *GetLinearPixels() { return linearEnabled ? linear.data() : nullptr; }
    bool SaveLinearImage(const char *filename) const { return linearEnabled && WritePFM(filename, linear.data(), width, height); }   // PFM
    // the first-hit feature planes (rt_outputs in rt_mi355x.h: normal, albedo, alpha, object id), row-major like GetPixels();
    // nothing is allocated until EnableFeatures() and the getters are NULL without it.  Renderer::BeginRender fills them
    // through rt_render_begin_outputs.  SaveFeatureImages writes <prefix>_normal.pfm, <prefix>_albedo.pfm (PFM),
    // <prefix>_alpha.pfm (one-channel PFM) and <prefix>_id.png (ObjectIdColor of the id).
    void EnableFeatures();
    bool FeaturesEnabled() const { return featuresEnabled; }
    float *GetNormals() { return featuresEnabled ? normals.data() : nullptr; }
    float *GetAlbedo() { return featuresEnabled ? albedo.data() : nullptr; }
    float *GetAlpha() { return featuresEnabled ? alpha.data() : nullptr; }
    int32_t *GetObjectIds() { return featuresEnabled ? objectIds.data() : nullptr; }
    static void ObjectIdColor(int32_t id, uint8_t rgb[3]);      // a fixed colour per id; -1 (no object) is black
    bool SaveFeatureImages(const char *prefix) const;
    // The denoiser of rt_mi355x.h ("denoising") over the finished frame: the linear plane filtered under the guidance of the
    // normal, albedo, z and object-id planes, on `device`.  Needs EnableLinear() AND EnableFeatures() before the render;
    // without them, or when the GPU call fails, it returns false and DenoiseError() says why.  params == NULL: the defaults
    // of rt_denoise_default_params.  The getters are NULL and the Save functions fail until a Denoise() has succeeded.
    bool Denoise(const rt_denoise_params *params = nullptr, int device = 0);
    // The variance plane (rt_mi355x.h, "the variance plane"): per channel the variance of the mean of the linear plane, row-major
    // like GetLinearPixels(); nothing is allocated until EnableVariance() and GetVariance() is NULL without it.
    // Renderer::BeginRender then renders through rt_render_begin_outputs_var.  SaveVarianceImage writes a three-channel PFM.
    void EnableVariance();
    bool VarianceEnabled() const { return varianceEnabled; }
    float *GetVariance() { return varianceEnabled ? variance.data() : nullptr; }
    bool SaveVarianceImage(const char *filename) const { return varianceEnabled && WritePFM(filename, variance.data(), width, height); }
    // Denoise() with each pixel's own standard error as its colour tolerance (rt_denoise_var_host; k_sigma standard errors):
    // needs EnableVariance() as well before the render.  Fills the same outputs as Denoise(), and GetDenoisedVariance().
    bool DenoiseGuided(const rt_denoise_params *params = nullptr, float k_sigma = 4.0f, int device = 0);
    float *GetDenoisedVariance() { return denoisedVariance.empty() ? nullptr : denoisedVariance.data(); }
    const std::string &DenoiseError() const { return denoiseError; }
    float *GetDenoisedPixels() { return denoised.empty() ? nullptr : denoised.data(); }         // linear float RGB
    uint8_t *GetDenoisedImage() { return denoisedImg.empty() ? nullptr : denoisedImg.data(); }  // Color24 after gamma
    bool SaveDenoisedImage(const char *filename) const { return !denoised.empty() && WritePFM(filename, denoised.data(), width, height); }    // PFM
    bool SaveDenoisedPNG(const char *filename) const { return !denoisedImg.empty() && WritePNG(filename, denoisedImg.data(), width, height, 3); }
    // Temporal accumulation (rt_mi355x.h, "temporal accumulation") over the frames of a STATIC scene: after each finished render
    // AccumulateTemporal(camera the frame was rendered with) blends the frame into the history, reprojected from the previous
    // call's camera.  Needs EnableTemporal(), EnableLinear() and EnableFeatures() before the render; with EnableVariance() the
    // variance is accumulated too (GetAccumulatedVariance()).  The history is created by the first call, on `device`, and lives
    // until the image is destroyed, Init() changes the size, or another device is named; ResetTemporal() makes the next frame
    // start from nothing.  false + TemporalError() on failure.  params == NULL: the defaults of rt_temporal_default_params.
    void EnableTemporal() { temporalEnabled = true; }
    bool TemporalEnabled() const { return temporalEnabled; }
    bool AccumulateTemporal(const Camera &camera, const rt_temporal_params *params = nullptr, int device = 0);
    // The same for a scene whose NODES may have moved since the previous frame (rt_mi355x.h, "motion vectors"): rt_motion from
    // the frame's z and object ids, the two cameras and the two lowered node arrays (rt::Lower's SceneData::nodes, n each;
    // prevNodes == NULL: nothing moved -- the first frame, with prevCamera = camera), then rt_temporal_motion with that plane.
    // The plane is kept next to the others: GetMotion(), (fx, fy, z_exp) per pixel, NULL until a call has succeeded.
    bool AccumulateTemporalMoving(const Camera &camera, const Camera &prevCamera, const rt_node *nodes, const rt_node *prevNodes, int n,
                                  const rt_temporal_params *params = nullptr, int device = 0);
    float *GetMotion() { return motion.empty() ? nullptr : motion.data(); }
    // History rectification (rt_mi355x.h, "history rectification"): from now on AccumulateTemporal() and
    // AccumulateTemporalMoving() clamp the reprojected history into the current frame's neighbourhood box
    // (rt_temporal_clip_host).  clip == NULL: the defaults of rt_temporal_clip_default; its out_clipped is ignored -- the mask is
    // kept next to the other planes: GetClipped(), float per pixel (0 no history, 1 kept, 2 clipped), NULL until a call has
    // succeeded.
    void EnableTemporalClip(const rt_temporal_clip *clip = nullptr);
    bool TemporalClipEnabled() const { return temporalClipEnabled; }
    float *GetClipped() { return clipped.empty() ? nullptr : clipped.data(); }
    void ResetTemporal();
    int TemporalFrames() const { return rt_history_frames(history); }
    const std::string &TemporalError() const { return temporalError; }
    float *GetAccumulatedPixels() { return accumulated.empty() ? nullptr : accumulated.data(); }                  // linear float RGB
    float *GetAccumulatedVariance() { return accumulatedVariance.empty() ? nullptr : accumulatedVariance.data(); }
    float *GetHistoryLength() { return historyLength.empty() ? nullptr : historyLength.data(); }                  // float per pixel
    bool SaveAccumulatedImage(const char *filename) const { return !accumulated.empty() && WritePFM(filename, accumulated.data(), width, height); }   // PFM
    // Exposure and tone mapping (rt_mi355x.h, "exposure and tone mapping") of the finished frame: ToneMap() meters, adapts the
    // exposure from the previous call's and tone-maps the most processed linear plane the image holds -- the denoised one, else
    // the accumulated one, else the render's -- with the object ids when EnableFeatures() was called (the background is then not
    // metered).  Needs EnableToneMap() and EnableLinear() before the render.  The rt_exposure is created by the first call, on
    // `device`, and lives until the image is destroyed or another device is named (it is not tied to a size: Init() keeps it);
    // ResetToneMap() makes the next frame the first again.  false + ToneMapError() on failure.  params == NULL: the defaults of
    // rt_tonemap_default_params.  The getters are NULL and SaveDisplayImage fails until a ToneMap() has succeeded.
    void EnableToneMap() { toneMapEnabled = true; }
    bool ToneMapEnabled() const { return toneMapEnabled; }
    bool ToneMap(const rt_tonemap_params *params = nullptr, int device = 0);
    void ResetToneMap();
    float ToneMapExposure() const;      // log2 of the scale the last METERED ToneMap() applied (auto_exposure != 0; 0 before the first)
    const std::string &ToneMapError() const { return toneMapError; }
    float *GetDisplayPixels() { return display.empty() ? nullptr : display.data(); }            // display-referred float RGB
    uint8_t *GetDisplayImage() { return displayImg.empty() ? nullptr : displayImg.data(); }     // Color24 after gamma
    bool SaveDisplayImage(const char *filename) const { return !displayImg.empty() && WritePNG(filename, displayImg.data(), width, height, 3); }
    // Bloom (rt_mi355x.h, "bloom"): from now on ToneMap() blooms the plane it would tone-map -- relative to the scale the exposure
    // state holds from the call before -- and tone-maps the result.  params == NULL: the defaults of rt_bloom_default_params.
    // The rt_bloom is created by the first ToneMap(), on its device, and lives until the image is destroyed, Init() changes the
    // size or another device is named.  GetBloomed() is the bloomed linear plane, NULL until a ToneMap() has succeeded with it.
    void EnableBloom(const rt_bloom_params *params = nullptr);
    bool BloomEnabled() const { return bloomEnabled; }
    float *GetBloomed() { return bloomed.empty() ? nullptr : bloomed.data(); }                  // linear float RGB
    bool SaveBloomedImage(const char *filename) const { return !bloomed.empty() && WritePFM(filename, bloomed.data(), width, height); }   // PFM
    // Motion blur (rt_mi355x.h, "motion blur"): from now on ToneMap() first blurs the plane it would bloom or tone-map, along the
    // motion plane of the last AccumulateTemporalMoving() and with the frame's z; bloom and the curve then work on the result.
    // Without such a plane (no moving accumulation yet, or a plain AccumulateTemporal() since) the stage is a no-op and
    // GetMotionBlurred() is NULL.  params == NULL: the defaults of rt_motion_blur_default_params.  The rt_motion_blur is created
    // by the first ToneMap() that needs it, on its device, and lives until the image is destroyed, Init() changes the size or
    // another device is named.
    void EnableMotionBlur(const rt_motion_blur_params *params = nullptr);
    bool MotionBlurEnabled() const { return motionBlurEnabled; }
    float *GetMotionBlurred() { return motionBlurred.empty() ? nullptr : motionBlurred.data(); }    // linear float RGB
    bool SaveMotionBlurredImage(const char *filename) const { return !motionBlurred.empty() && WritePFM(filename, motionBlurred.data(), width, height); }   // PFM
    // Depth of field (rt_mi355x.h, "depth of field"): the lens as an image-space stage.  Render with the scene camera's dof set to 0
    // (exact planes), run Denoise() / AccumulateTemporal() as wanted, then DepthOfField(camera) with the camera WITH its dof: the
    // most processed linear plane the image holds -- the denoised one, else the accumulated one, else the render's -- is defocused
    // from the z-buffer.  From then on ToneMap() starts from the defocused plane (ahead of motion blur, bloom and the curve),
    // until a new Denoise(), accumulation or Init() discards it: the order of stages is denoise / accumulate -> depth of field
    // -> motion blur -> bloom -> tone map.  Needs EnableDepthOfField() and EnableLinear() before the render.  params == NULL: the
    // defaults of rt_dof_default_params.  The rt_dof is created by the first call, on `device`, and lives until the image is
    // destroyed, Init() changes the size or another device is named.  false + DepthOfFieldError() on failure.  GetDefocused() is
    // linear float RGB and GetCoc() the signed circle of confusion in pixels, both NULL until a call has succeeded.
    void EnableDepthOfField(const rt_dof_params *params = nullptr);
    bool DepthOfFieldEnabled() const { return dofEnabled; }
    bool DepthOfField(const Camera &camera, int device = 0);
    const std::string &DepthOfFieldError() const { return dofError; }
    float *GetDefocused() { return defocused.empty() ? nullptr : defocused.data(); }            // linear float RGB
    float *GetCoc() { return coc.empty() ? nullptr : coc.data(); }                              // float per pixel
    bool SaveDefocusedImage(const char *filename) const { return !defocused.empty() && WritePFM(filename, defocused.data(), width, height); }   // PFM
    int GetNumRenderedPixels() const;
    bool IsRenderDone() const { return GetNumRenderedPixels() >= width * height; }
    void ComputeZBufferImage();        // scene.h:591-613
    int ComputeSampleCountImage();     // scene.h:615-637
    bool SaveImage(const char *filename) const { return WritePNG(filename, img.data(), width, height, 3); }
    bool SaveZImage(const char *filename) const { return WritePNG(filename, zbufferImg.data(), width, height, 1); }
    bool SaveSampleCountImage(const char *filename) const { return WritePNG(filename, sampleCountImg.data(), width, height, 1); }
    void AttachJob(rt_job *j) { jobs.push_back(j); }
    void DetachJobs(int pixels) { jobs.clear(); finalPixels = pixels; }
};

class Renderer {
public:
    Scene scene;                 // rootNode, camera, materials, lights, objList, environment, background
    RenderImage renderImage;
    rt_params params;            // the reference's #defines as run-time values (incl. MAX_NUM_OF_PHOTON / PHOTON_BOUNCE)
    // devices to render on: empty (the default) = every gfx950 device of the node (rt_device_count()).  The reference spreads
    // the pixels over 2 x hardware_concurrency threads that share one counter (FIN/main.cpp:71-78, 987-997); here device r of
    // N takes the interleaved 32 x 8 tiles r, r+N, ... and writes them into the same RenderImage.
    std::vector<int> devices;
    std::string photonDump;      // where generatePhotonMap's .dat goes (FIN/main.cpp:398 hard-codes a path); empty = no dump
    uint32_t renderFlags = 0;    // rt_scene_set_render_flags at BeginRender: 0, or RT_RENDER_REPRODUCIBLE (byte-identical renders)

    Renderer();
    ~Renderer();
    int LoadScene(const char *filename);          // FIN/xmlload.cpp:65-132: 1 on success, 0 on failure
    // balanced photon array (index 0 unused), the product of generatePhotonMap (FIN/main.cpp:350-402)
    bool SetPhotonMap(const rt_photon *balanced, uint32_t n_stored);
    // Like the reference's (FIN/main.cpp:984-998): generatePhotonMap first -- when no map was set with SetPhotonMap and the
    // FIN model renders -- then the workers; but BOTH on background threads, so the call returns immediately (progress stays
    // 0 while the photon pass runs).  false + LastError() when the GPU path cannot start.
    bool BeginRender();
    void StopRender();
    bool WaitRender();           // joins the background job (the reference polls IsRenderDone instead)
    void saveImage(const char *image = "prj13box.png", const char *samples = "prj13box_sc.png", const char *zimage = nullptr);
    const std::string &LastError() const { return error; }
    const rt_stats &Stats() const { return stats; }         // summed over the devices
    const rt_setup_ms &PhotonPassMs() const { return setup; }   // stage times of the photon pass BeginRender ran (zero: none)
    int NumDevices() const { return (int)jobs.size(); }
private:
    rt_scene *handle = nullptr;
    std::vector<rt_job *> jobs;
    rt_setup_ms setup{};
    std::string error;
    rt_stats stats{};
    bool lowered = false;
};

}  // namespace rt
#endif
