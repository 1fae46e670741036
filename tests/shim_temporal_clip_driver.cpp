// shim_temporal_clip_driver.cpp -- test infrastructure: rt::RenderImage::EnableTemporalClip() / GetClipped() on top of
// EnableTemporal() / AccumulateTemporal().  Loads the scene file, checks that no mask exists before EnableTemporalClip(), then
// renders two frames in reproducible mode with the linear, feature and variance planes -- the second with another seed and the
// camera moved by (0.3, 0, 0.1) -- and accumulates each with the default parameters and the default rectification.  The test
// compares what is saved with Scene.render_temporal(clip=True) of the same two frames.  Built by tests/test_temporal_clip.py:
// without a GPU only the build is checked.
//   shim_temporal_clip_driver <scene.xml> <prefix> <width> <height>
// writes <prefix>_acc1.pfm, <prefix>_acc2.pfm (the accumulated colour after each frame), <prefix>_len2.pfm and
// <prefix>_clip2.pfm (the one-channel history length and mask after the second).
// Renders with the P13 model, adaptive 4 -> 8, no photon pass, seeds 11 and 12.
#include <cstdlib>

#include "shim_driver_util.h"

int main(int argc, char **argv)
{
    if (argc < 5) { fprintf(stderr, "usage: shim_temporal_clip_driver scene.xml prefix w h\n"); return 2; }
    rt::Renderer r;
    if (!r.LoadScene(argv[1])) { fprintf(stderr, "LoadScene failed: %s\n", r.LastError().c_str()); return 3; }
    rt::RenderImage &img = r.renderImage;
    const std::string prefix(argv[2]);
    if (img.TemporalClipEnabled() || img.GetClipped()) { fprintf(stderr, "a mask exists before EnableTemporalClip()\n"); return 7; }
    r.scene.camera.imgWidth = atoi(argv[3]); r.scene.camera.imgHeight = atoi(argv[4]);
    r.params.shade_model = RT_SHADE_P13; r.params.bounce = 6; r.params.photon_count = 0;
    r.params.min_sample = 4; r.params.max_sample = 8; r.params.threshold = 1e-3f;
    r.renderFlags = RT_RENDER_REPRODUCIBLE;
    img.Init(r.scene.camera.imgWidth, r.scene.camera.imgHeight);
    img.EnableLinear();
    img.EnableFeatures();
    img.EnableVariance();
    img.EnableTemporal();
    rt_temporal_clip bad;
    rt_temporal_clip_default(&bad);
    bad.radius = 4;
    img.EnableTemporalClip(&bad);
    r.params.seed = 11;
    if (!render(r)) return 4;
    if (img.AccumulateTemporal(r.scene.camera) || img.TemporalError().find("radius") == std::string::npos || img.TemporalFrames() != 0) {
        fprintf(stderr, "a radius of 4 was not refused\n");
        return 7;
    }
    img.EnableTemporalClip();
    if (!img.TemporalClipEnabled()) return 7;
    if (!img.AccumulateTemporal(r.scene.camera) || img.TemporalFrames() != 1 || !img.GetClipped()) { fprintf(stderr, "AccumulateTemporal failed: %s\n", img.TemporalError().c_str()); return 8; }
    if (!img.SaveAccumulatedImage((prefix + "_acc1.pfm").c_str())) { fprintf(stderr, "saving failed\n"); return 9; }
    r.scene.camera.pos.x += 0.3f; r.scene.camera.pos.z += 0.1f;
    r.params.seed = 12;
    if (!render(r)) return 4;
    if (!img.AccumulateTemporal(r.scene.camera) || img.TemporalFrames() != 2) { fprintf(stderr, "AccumulateTemporal failed: %s\n", img.TemporalError().c_str()); return 8; }
    if (!img.GetAccumulatedPixels() || !img.GetHistoryLength() || !img.GetClipped()) { fprintf(stderr, "AccumulateTemporal() left no planes\n"); return 8; }
    if (!img.SaveAccumulatedImage((prefix + "_acc2.pfm").c_str()) ||
        !rt::WritePFM((prefix + "_len2.pfm").c_str(), img.GetHistoryLength(), img.GetWidth(), img.GetHeight(), 1) ||
        !rt::WritePFM((prefix + "_clip2.pfm").c_str(), img.GetClipped(), img.GetWidth(), img.GetHeight(), 1)) {
        fprintf(stderr, "saving failed\n");
        return 9;
    }
    img.ResetTemporal();
    if (img.GetClipped() || img.TemporalFrames() != 0) { fprintf(stderr, "ResetTemporal() left a mask\n"); return 8; }
    printf("pixels %d of %d frames 2\n", img.GetNumRenderedPixels(), img.GetWidth() * img.GetHeight());
    return 0;
}
