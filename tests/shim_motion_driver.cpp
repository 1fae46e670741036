// shim_motion_driver.cpp -- test infrastructure: rt::RenderImage::AccumulateTemporalMoving() / GetMotion().  Loads the scene
// file and renders two frames in reproducible mode with the linear, feature and variance planes -- the second with another seed
// and the node <child> (an index into the root's children) translated by (dx, dy, dz), under the same camera -- and accumulates
// each with the default parameters: the first with prevNodes = NULL, the second with the first frame's lowered nodes.  The test
// compares what is saved with Scene.render_temporal(moving=True) of the same two frames.  Built by tests/test_motion.py: without
// a GPU only the build is checked.
//   shim_motion_driver <scene.xml> <prefix> <width> <height> <child> <dx> <dy> <dz>
// writes <prefix>_mv1.pfm, <prefix>_mv2.pfm (the motion plane of each frame), <prefix>_acc2.pfm and <prefix>_len2.pfm (the
// accumulated colour and the one-channel history length after the second).
// Renders with the P13 model, adaptive 4 -> 8, no photon pass, seeds 11 and 12.
#include <cstdlib>

#include "shim_driver_util.h"

int main(int argc, char **argv)
{
    if (argc < 9) { fprintf(stderr, "usage: shim_motion_driver scene.xml prefix w h child dx dy dz\n"); return 2; }
    rt::Renderer r;
    if (!r.LoadScene(argv[1])) { fprintf(stderr, "LoadScene failed: %s\n", r.LastError().c_str()); return 3; }
    rt::RenderImage &img = r.renderImage;
    const std::string prefix(argv[2]);
    const int child = atoi(argv[5]);
    if (child < 0 || child >= r.scene.rootNode.GetNumChild()) { fprintf(stderr, "the root has no child %d\n", child); return 3; }
    r.scene.camera.imgWidth = atoi(argv[3]); r.scene.camera.imgHeight = atoi(argv[4]);
    r.params.shade_model = RT_SHADE_P13; r.params.bounce = 6; r.params.photon_count = 0;
    r.params.min_sample = 4; r.params.max_sample = 8; r.params.threshold = 1e-3f;
    r.renderFlags = RT_RENDER_REPRODUCIBLE;
    img.Init(r.scene.camera.imgWidth, r.scene.camera.imgHeight);
    img.EnableLinear();
    img.EnableFeatures();
    img.EnableVariance();
    img.EnableTemporal();
    if (img.GetMotion()) { fprintf(stderr, "a motion plane exists before AccumulateTemporalMoving()\n"); return 7; }
    std::string err;
    rt::SceneData first, second;
    if (!rt::Lower(r.scene, first, &err)) { fprintf(stderr, "Lower failed: %s\n", err.c_str()); return 3; }
    r.params.seed = 11;
    if (!render(r)) return 4;
    if (!img.AccumulateTemporalMoving(r.scene.camera, r.scene.camera, first.nodes.data(), nullptr, (int)first.nodes.size()) || !img.GetMotion()) {
        fprintf(stderr, "AccumulateTemporalMoving failed: %s\n", img.TemporalError().c_str());
        return 8;
    }
    if (!rt::WritePFM((prefix + "_mv1.pfm").c_str(), img.GetMotion(), img.GetWidth(), img.GetHeight())) { fprintf(stderr, "saving failed\n"); return 9; }
    r.scene.rootNode.GetChild(child)->Translate(rt::Point3((float)atof(argv[6]), (float)atof(argv[7]), (float)atof(argv[8])));
    if (!rt::Lower(r.scene, second, &err)) { fprintf(stderr, "Lower failed: %s\n", err.c_str()); return 3; }
    r.params.seed = 12;
    if (!render(r)) return 4;
    if (!img.AccumulateTemporalMoving(r.scene.camera, r.scene.camera, second.nodes.data(), first.nodes.data(), (int)second.nodes.size()) ||
        img.TemporalFrames() != 2) {
        fprintf(stderr, "AccumulateTemporalMoving failed: %s\n", img.TemporalError().c_str());
        return 8;
    }
    if (!rt::WritePFM((prefix + "_mv2.pfm").c_str(), img.GetMotion(), img.GetWidth(), img.GetHeight()) ||
        !img.SaveAccumulatedImage((prefix + "_acc2.pfm").c_str()) ||
        !rt::WritePFM((prefix + "_len2.pfm").c_str(), img.GetHistoryLength(), img.GetWidth(), img.GetHeight(), 1)) {
        fprintf(stderr, "saving failed\n");
        return 9;
    }
    img.ResetTemporal();
    if (img.GetMotion() || img.TemporalFrames() != 0) { fprintf(stderr, "ResetTemporal() left a motion plane\n"); return 8; }
    printf("pixels %d of %d nodes %d frames 2\n", img.GetNumRenderedPixels(), img.GetWidth() * img.GetHeight(), (int)second.nodes.size());
    return 0;
}
