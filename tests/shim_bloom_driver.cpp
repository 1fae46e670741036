// shim_bloom_driver.cpp -- test infrastructure: rt::RenderImage::EnableBloom() / GetBloomed() / SaveBloomedImage().  Loads the
// scene file, checks that nothing exists before EnableBloom(), then renders two frames in reproducible mode with the linear and
// feature planes -- the second with another seed -- and tone-maps each with the default parameters: the first frame is bloomed
// relative to 2^0 (the state holds no metered frame yet), the second relative to the exposure the first one left.  The test
// compares what is saved with capi.Bloom.apply / capi.Exposure.tonemap of Scene.render_outputs' planes of the same two frames.
// Built by tests/test_bloom.py: without a GPU only the build is checked.
//   shim_bloom_driver <scene.xml> <prefix> <width> <height>
// writes <prefix>_bloom1.pfm, <prefix>_bloom2.pfm (SaveBloomedImage) and <prefix>_rgb1.bin, <prefix>_rgb2.bin (the Color24 bytes
// of the display image as they are in memory).
// Renders with the P13 model, adaptive 4 -> 8, no photon pass, seeds 11 and 12; bloom with threshold 0.5 and intensity 0.5.
#include <cstdlib>

#include "shim_driver_util.h"

int main(int argc, char **argv)
{
    if (argc < 5) { fprintf(stderr, "usage: shim_bloom_driver scene.xml prefix w h\n"); return 2; }
    rt::Renderer r;
    if (!r.LoadScene(argv[1])) { fprintf(stderr, "LoadScene failed: %s\n", r.LastError().c_str()); return 3; }
    rt::RenderImage &img = r.renderImage;
    const std::string prefix(argv[2]);
    if (img.BloomEnabled() || img.GetBloomed() || img.SaveBloomedImage((prefix + "_bloom1.pfm").c_str())) {
        fprintf(stderr, "a bloomed image exists before EnableBloom()\n");
        return 7;
    }
    r.scene.camera.imgWidth = atoi(argv[3]); r.scene.camera.imgHeight = atoi(argv[4]);
    r.params.shade_model = RT_SHADE_P13; r.params.bounce = 6; r.params.photon_count = 0;
    r.params.min_sample = 4; r.params.max_sample = 8; r.params.threshold = 1e-3f;
    r.renderFlags = RT_RENDER_REPRODUCIBLE;
    img.Init(r.scene.camera.imgWidth, r.scene.camera.imgHeight);
    img.EnableLinear();
    img.EnableFeatures();
    img.EnableToneMap();
    rt_bloom_params bp;
    rt_bloom_default_params(&bp);
    bp.threshold = 0.5f; bp.intensity = 0.5f;
    img.EnableBloom(&bp);
    const size_t n = (size_t)img.GetWidth() * img.GetHeight();
    for (int frame = 1; frame <= 2; frame++) {
        const std::string k = std::to_string(frame);
        r.params.seed = 10 + frame;
        if (!render(r)) return 4;
        if (!img.ToneMap()) { fprintf(stderr, "ToneMap failed: %s\n", img.ToneMapError().c_str()); return 8; }
        if (!img.GetBloomed() || !img.SaveBloomedImage((prefix + "_bloom" + k + ".pfm").c_str()) ||
            !dump(prefix + "_rgb" + k + ".bin", img.GetDisplayImage(), n * 3)) { fprintf(stderr, "saving failed\n"); return 9; }
    }
    printf("pixels %d of %d exposure %.9g\n", img.GetNumRenderedPixels(), img.GetWidth() * img.GetHeight(), img.ToneMapExposure());
    return 0;
}
