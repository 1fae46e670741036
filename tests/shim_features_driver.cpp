// shim_features_driver.cpp -- test infrastructure: rt::Renderer with the opt-in first-hit feature planes.  Loads the scene
// file, checks that nothing exists before EnableFeatures(), sets the view the test asks for, then EnableFeatures() +
// BeginRender() + WaitRender() and SaveFeatureImages(prefix).  Built by tests/test_feature_planes.py: without a GPU only
// the build is checked, on the GPU the saved files are compared with a render through the C ABI.
//   shim_features_driver <scene.xml> <prefix> <width> <height> <fov> <bg r> <bg g> <bg b> <min_sample> <max_sample> <threshold>
// Renders with the P13 model, no photon pass, black environment.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../raytracing_folder_amd/csrc/host/rt_shim.h"

int main(int argc, char **argv)
{
    if (argc < 12) { fprintf(stderr, "usage: shim_features_driver scene.xml prefix w h fov bgr bgg bgb min max threshold\n"); return 2; }
    rt::Renderer r;
    if (!r.LoadScene(argv[1])) { fprintf(stderr, "LoadScene failed: %s\n", r.LastError().c_str()); return 3; }
    rt::RenderImage &img = r.renderImage;
    if (img.GetNormals() || img.GetAlbedo() || img.GetAlpha() || img.GetObjectIds() || img.SaveFeatureImages(argv[2])) {
        fprintf(stderr, "feature planes exist before EnableFeatures()\n");
        return 7;
    }
    r.scene.camera.imgWidth = atoi(argv[3]); r.scene.camera.imgHeight = atoi(argv[4]); r.scene.camera.fov = (float)atof(argv[5]);
    r.scene.background.SetColor(rt::Color((float)atof(argv[6]), (float)atof(argv[7]), (float)atof(argv[8])));
    r.scene.environment.SetColor(rt::Color(0, 0, 0));
    r.params.shade_model = RT_SHADE_P13; r.params.bounce = 6; r.params.photon_count = 0;
    r.params.min_sample = atoi(argv[9]); r.params.max_sample = atoi(argv[10]); r.params.threshold = (float)atof(argv[11]);
    img.Init(r.scene.camera.imgWidth, r.scene.camera.imgHeight);
    img.EnableFeatures();
    const int n = img.GetWidth() * img.GetHeight();
    if (!img.GetNormals() || !img.GetAlbedo() || !img.GetAlpha() || !img.GetObjectIds()) { fprintf(stderr, "EnableFeatures() left no planes\n"); return 8; }
    for (int i = 0; i < n; i++) { img.GetAlpha()[i] = -1.0f; img.GetObjectIds()[i] = -2; }        // every pixel must be written by the render
    if (!r.BeginRender()) { fprintf(stderr, "BeginRender failed: %s\n", r.LastError().c_str()); return 4; }
    const int devices = r.NumDevices();
    if (!r.WaitRender()) { fprintf(stderr, "render failed: %s\n", r.LastError().c_str()); return 6; }
    int untouched = 0;
    for (int i = 0; i < n; i++) untouched += (img.GetAlpha()[i] == -1.0f) + (img.GetObjectIds()[i] == -2);
    if (!img.SaveFeatureImages(argv[2])) { fprintf(stderr, "SaveFeatureImages failed\n"); return 9; }
    printf("devices %d pixels %d of %d untouched %d\n", devices, img.GetNumRenderedPixels(), n, untouched);
    return 0;
}
