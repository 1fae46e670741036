// shim_temporal_driver.cpp -- test infrastructure: rt::RenderImage::EnableTemporal() / AccumulateTemporal() / ResetTemporal() /
// SaveAccumulatedImage().  Loads the scene file, checks that nothing exists before EnableTemporal() and that
// AccumulateTemporal() refuses a frame without it, then renders two frames in reproducible mode with the linear, feature and
// variance planes -- the second with another seed and the camera moved by (0.3, 0, 0.1) -- and accumulates each with the default
// parameters.  The test compares what is saved with capi.History.accumulate of Scene.render_outputs' planes of the same two
// frames.  Built by tests/test_temporal.py: without a GPU only the build is checked.
//   shim_temporal_driver <scene.xml> <prefix> <width> <height>
// writes <prefix>_acc1.pfm, <prefix>_acc2.pfm (the accumulated colour after each frame), <prefix>_accvar2.pfm and
// <prefix>_len2.pfm (the accumulated variance and the one-channel history length after the second).
// Renders with the P13 model, adaptive 4 -> 8, no photon pass, seeds 11 and 12.
#include <cstdlib>

#include "shim_driver_util.h"

int main(int argc, char **argv)
{
    if (argc < 5) { fprintf(stderr, "usage: shim_temporal_driver scene.xml prefix w h\n"); return 2; }
    rt::Renderer r;
    if (!r.LoadScene(argv[1])) { fprintf(stderr, "LoadScene failed: %s\n", r.LastError().c_str()); return 3; }
    rt::RenderImage &img = r.renderImage;
    const std::string prefix(argv[2]);
    if (img.TemporalEnabled() || img.GetAccumulatedPixels() || img.TemporalFrames() != 0 || img.SaveAccumulatedImage((prefix + "_acc1.pfm").c_str())) {
        fprintf(stderr, "an accumulated frame exists before EnableTemporal()\n");
        return 7;
    }
    r.scene.camera.imgWidth = atoi(argv[3]); r.scene.camera.imgHeight = atoi(argv[4]);
    r.params.shade_model = RT_SHADE_P13; r.params.bounce = 6; r.params.photon_count = 0;
    r.params.min_sample = 4; r.params.max_sample = 8; r.params.threshold = 1e-3f;
    r.renderFlags = RT_RENDER_REPRODUCIBLE;
    img.Init(r.scene.camera.imgWidth, r.scene.camera.imgHeight);
    img.EnableLinear();
    img.EnableFeatures();
    img.EnableVariance();
    if (img.AccumulateTemporal(r.scene.camera) || img.TemporalError().empty()) { fprintf(stderr, "AccumulateTemporal() worked without EnableTemporal()\n"); return 7; }
    img.EnableTemporal();
    r.params.seed = 11;
    if (!render(r)) return 4;
    if (!img.AccumulateTemporal(r.scene.camera)) { fprintf(stderr, "AccumulateTemporal failed: %s\n", img.TemporalError().c_str()); return 8; }
    img.ResetTemporal();                                    // and once more from nothing: the same first frame
    if (img.GetAccumulatedPixels() || img.TemporalFrames() != 0) { fprintf(stderr, "ResetTemporal() left a frame\n"); return 8; }
    if (!img.AccumulateTemporal(r.scene.camera) || img.TemporalFrames() != 1) { fprintf(stderr, "AccumulateTemporal failed after the reset: %s\n", img.TemporalError().c_str()); return 8; }
    if (!img.SaveAccumulatedImage((prefix + "_acc1.pfm").c_str())) { fprintf(stderr, "saving failed\n"); return 9; }
    r.scene.camera.pos.x += 0.3f; r.scene.camera.pos.z += 0.1f;
    r.params.seed = 12;
    if (!render(r)) return 4;
    if (!img.AccumulateTemporal(r.scene.camera) || img.TemporalFrames() != 2) { fprintf(stderr, "AccumulateTemporal failed: %s\n", img.TemporalError().c_str()); return 8; }
    if (!img.GetAccumulatedPixels() || !img.GetAccumulatedVariance() || !img.GetHistoryLength()) { fprintf(stderr, "AccumulateTemporal() left no planes\n"); return 8; }
    if (!img.SaveAccumulatedImage((prefix + "_acc2.pfm").c_str()) ||
        !rt::WritePFM((prefix + "_accvar2.pfm").c_str(), img.GetAccumulatedVariance(), img.GetWidth(), img.GetHeight()) ||
        !rt::WritePFM((prefix + "_len2.pfm").c_str(), img.GetHistoryLength(), img.GetWidth(), img.GetHeight(), 1)) {
        fprintf(stderr, "saving failed\n");
        return 9;
    }
    printf("pixels %d of %d frames %d\n", img.GetNumRenderedPixels(), img.GetWidth() * img.GetHeight(), img.TemporalFrames());
    return 0;
}
