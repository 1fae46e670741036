// shim_tonemap_driver.cpp -- test infrastructure: rt::RenderImage::EnableToneMap() / ToneMap() / ResetToneMap() /
// SaveDisplayImage().  Loads the scene file, checks that nothing exists before EnableToneMap() and that ToneMap() refuses a
// frame without it, then renders two frames in reproducible mode with the linear and feature planes -- the second with another
// seed -- and tone-maps each: the first with the default parameters, the second with REINHARD and adapt_up = adapt_down = 0.5.
// The test compares what is saved with capi.Exposure.tonemap of Scene.render_outputs' planes of the same two frames.  Built by
// tests/test_tonemap.py: without a GPU only the build is checked.
//   shim_tonemap_driver <scene.xml> <prefix> <width> <height>
// writes <prefix>_disp1.pfm, <prefix>_disp2.pfm (the float display planes), <prefix>_rgb1.bin, <prefix>_rgb2.bin (the Color24
// bytes as they are in memory) and <prefix>_2.png (SaveDisplayImage).
// Renders with the P13 model, adaptive 4 -> 8, no photon pass, seeds 11 and 12.
#include <cstdlib>

#include "shim_driver_util.h"

int main(int argc, char **argv)
{
    if (argc < 5) { fprintf(stderr, "usage: shim_tonemap_driver scene.xml prefix w h\n"); return 2; }
    rt::Renderer r;
    if (!r.LoadScene(argv[1])) { fprintf(stderr, "LoadScene failed: %s\n", r.LastError().c_str()); return 3; }
    rt::RenderImage &img = r.renderImage;
    const std::string prefix(argv[2]);
    if (img.ToneMapEnabled() || img.GetDisplayPixels() || img.GetDisplayImage() || img.SaveDisplayImage((prefix + "_2.png").c_str())) {
        fprintf(stderr, "a display image exists before EnableToneMap()\n");
        return 7;
    }
    r.scene.camera.imgWidth = atoi(argv[3]); r.scene.camera.imgHeight = atoi(argv[4]);
    r.params.shade_model = RT_SHADE_P13; r.params.bounce = 6; r.params.photon_count = 0;
    r.params.min_sample = 4; r.params.max_sample = 8; r.params.threshold = 1e-3f;
    r.renderFlags = RT_RENDER_REPRODUCIBLE;
    img.Init(r.scene.camera.imgWidth, r.scene.camera.imgHeight);
    img.EnableLinear();
    img.EnableFeatures();
    if (img.ToneMap() || img.ToneMapError().empty()) { fprintf(stderr, "ToneMap() worked without EnableToneMap()\n"); return 7; }
    img.EnableToneMap();
    const size_t n = (size_t)img.GetWidth() * img.GetHeight();
    r.params.seed = 11;
    if (!render(r)) return 4;
    if (!img.ToneMap()) { fprintf(stderr, "ToneMap failed: %s\n", img.ToneMapError().c_str()); return 8; }
    img.ResetToneMap();                                     // and once more from nothing: the same first frame
    if (img.GetDisplayPixels() || img.GetDisplayImage()) { fprintf(stderr, "ResetToneMap() left a frame\n"); return 8; }
    if (!img.ToneMap()) { fprintf(stderr, "ToneMap failed after the reset: %s\n", img.ToneMapError().c_str()); return 8; }
    const float e1 = img.ToneMapExposure();
    if (!rt::WritePFM((prefix + "_disp1.pfm").c_str(), img.GetDisplayPixels(), img.GetWidth(), img.GetHeight()) ||
        !dump(prefix + "_rgb1.bin", img.GetDisplayImage(), n * 3)) { fprintf(stderr, "saving failed\n"); return 9; }
    r.params.seed = 12;
    if (!render(r)) return 4;
    rt_tonemap_params p;
    rt_tonemap_default_params(&p);
    p.op = RT_TONEMAP_REINHARD; p.adapt_up = 0.5f; p.adapt_down = 0.5f;
    if (!img.ToneMap(&p)) { fprintf(stderr, "ToneMap failed: %s\n", img.ToneMapError().c_str()); return 8; }
    if (!rt::WritePFM((prefix + "_disp2.pfm").c_str(), img.GetDisplayPixels(), img.GetWidth(), img.GetHeight()) ||
        !dump(prefix + "_rgb2.bin", img.GetDisplayImage(), n * 3) || !img.SaveDisplayImage((prefix + "_2.png").c_str())) {
        fprintf(stderr, "saving failed\n");
        return 9;
    }
    printf("pixels %d of %d exposure %.9g %.9g\n", img.GetNumRenderedPixels(), img.GetWidth() * img.GetHeight(), e1, img.ToneMapExposure());
    return 0;
}
