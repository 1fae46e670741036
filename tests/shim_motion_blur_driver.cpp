// shim_motion_blur_driver.cpp -- test infrastructure: rt::RenderImage::EnableMotionBlur() / GetMotionBlurred() /
// SaveMotionBlurredImage().  Loads the scene file and renders two frames in reproducible mode with the linear, feature and variance
// planes -- the second with another seed and the node <child> (an index into the root's children) translated by (dx, dy, dz), under
// the same camera -- accumulates each with AccumulateTemporalMoving() and the default parameters, and tone-maps each.  Before the
// first accumulation there is no motion plane: ToneMap() must leave no blurred plane.  The test compares what is saved with
// Scene.render_temporal(moving=True, denoise=False, motion_blur=) of the same two frames.  Built by tests/test_motion_blur.py:
// without a GPU only the build is checked.
//   shim_motion_blur_driver <scene.xml> <prefix> <width> <height> <child> <dx> <dy> <dz>
// writes <prefix>_mb1.pfm, <prefix>_mb2.pfm (SaveMotionBlurredImage after each frame) and <prefix>_acc2.pfm (the plane the second
// was made from).
// Renders with the P13 model, adaptive 4 -> 8, no photon pass, seeds 11 and 12; motion blur with shutter 1 and max_blur 8.
#include <cstdlib>

#include "shim_driver_util.h"

int main(int argc, char **argv)
{
    if (argc < 9) { fprintf(stderr, "usage: shim_motion_blur_driver scene.xml prefix w h child dx dy dz\n"); return 2; }
    rt::Renderer r;
    if (!r.LoadScene(argv[1])) { fprintf(stderr, "LoadScene failed: %s\n", r.LastError().c_str()); return 3; }
    rt::RenderImage &img = r.renderImage;
    const std::string prefix(argv[2]);
    const int child = atoi(argv[5]);
    if (child < 0 || child >= r.scene.rootNode.GetNumChild()) { fprintf(stderr, "the root has no child %d\n", child); return 3; }
    if (img.MotionBlurEnabled() || img.GetMotionBlurred() || img.SaveMotionBlurredImage((prefix + "_mb1.pfm").c_str())) {
        fprintf(stderr, "a blurred image exists before EnableMotionBlur()\n");
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
    img.EnableTemporal();
    img.EnableToneMap();
    rt_motion_blur_params mp;
    rt_motion_blur_default_params(&mp);
    mp.shutter = 1.0f; mp.max_blur = 8;
    img.EnableMotionBlur(&mp);
    std::string err;
    rt::SceneData first, second;
    if (!rt::Lower(r.scene, first, &err)) { fprintf(stderr, "Lower failed: %s\n", err.c_str()); return 3; }
    r.params.seed = 11;
    if (!render(r)) return 4;
    // no motion plane yet: the stage is a no-op
    if (!img.ToneMap() || img.GetMotionBlurred()) { fprintf(stderr, "ToneMap without a motion plane: %s\n", img.ToneMapError().c_str()); return 8; }
    if (!img.AccumulateTemporalMoving(r.scene.camera, r.scene.camera, first.nodes.data(), nullptr, (int)first.nodes.size())) {
        fprintf(stderr, "AccumulateTemporalMoving failed: %s\n", img.TemporalError().c_str());
        return 8;
    }
    if (!img.ToneMap() || !img.GetMotionBlurred() || !img.SaveMotionBlurredImage((prefix + "_mb1.pfm").c_str())) {
        fprintf(stderr, "ToneMap failed: %s\n", img.ToneMapError().c_str());
        return 8;
    }
    r.scene.rootNode.GetChild(child)->Translate(rt::Point3((float)atof(argv[6]), (float)atof(argv[7]), (float)atof(argv[8])));
    if (!rt::Lower(r.scene, second, &err)) { fprintf(stderr, "Lower failed: %s\n", err.c_str()); return 3; }
    r.params.seed = 12;
    if (!render(r)) return 4;
    if (!img.AccumulateTemporalMoving(r.scene.camera, r.scene.camera, second.nodes.data(), first.nodes.data(), (int)second.nodes.size())) {
        fprintf(stderr, "AccumulateTemporalMoving failed: %s\n", img.TemporalError().c_str());
        return 8;
    }
    if (!img.ToneMap() || !img.GetMotionBlurred() || !img.SaveMotionBlurredImage((prefix + "_mb2.pfm").c_str()) ||
        !img.SaveAccumulatedImage((prefix + "_acc2.pfm").c_str())) {
        fprintf(stderr, "ToneMap or saving failed: %s\n", img.ToneMapError().c_str());
        return 9;
    }
    printf("pixels %d of %d frames 2\n", img.GetNumRenderedPixels(), img.GetWidth() * img.GetHeight());
    return 0;
}
