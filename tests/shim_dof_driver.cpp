// shim_dof_driver.cpp -- test infrastructure: rt::RenderImage::EnableDepthOfField() / DepthOfField() / GetDefocused() / GetCoc() /
// SaveDefocusedImage().  Loads the scene file, renders one frame PINHOLE (the scene camera's dof set to 0) in reproducible mode with
// the linear and feature planes, denoises it with the default parameters, defocuses the denoised plane with the camera's lens
// (focaldist and dof from the command line) and tone-maps the result.  The test compares what is saved with
// Scene.render_denoised(depth_of_field=) of the same frame.  Built by tests/test_dof.py: without a GPU only the build is checked.
//   shim_dof_driver <scene.xml> <prefix> <width> <height> <focaldist> <dof> <max_coc>
// writes <prefix>_den.pfm (the plane the stage was given), <prefix>_dof.pfm (SaveDefocusedImage) and <prefix>_coc.pfm (GetCoc, one
// channel).
// Renders with the P13 model, adaptive 4 -> 8, no photon pass, seed 11.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../raytracing_folder_amd/csrc/host/rt_shim.h"

int main(int argc, char **argv)
{
    if (argc < 8) { fprintf(stderr, "usage: shim_dof_driver scene.xml prefix w h focaldist dof max_coc\n"); return 2; }
    rt::Renderer r;
    if (!r.LoadScene(argv[1])) { fprintf(stderr, "LoadScene failed: %s\n", r.LastError().c_str()); return 3; }
    rt::RenderImage &img = r.renderImage;
    const std::string prefix(argv[2]);
    if (img.DepthOfFieldEnabled() || img.GetDefocused() || img.GetCoc() || img.SaveDefocusedImage((prefix + "_dof.pfm").c_str())) {
        fprintf(stderr, "a defocused image exists before EnableDepthOfField()\n");
        return 7;
    }
    r.scene.camera.imgWidth = atoi(argv[3]); r.scene.camera.imgHeight = atoi(argv[4]);
    r.scene.camera.focaldist = (float)atof(argv[5]);
    r.scene.camera.dof = 0.0f;                                  // the render is pinhole: exact planes
    rt::Camera lens = r.scene.camera;
    lens.dof = (float)atof(argv[6]);
    r.params.shade_model = RT_SHADE_P13; r.params.bounce = 6; r.params.photon_count = 0;
    r.params.min_sample = 4; r.params.max_sample = 8; r.params.threshold = 1e-3f; r.params.seed = 11;
    r.renderFlags = RT_RENDER_REPRODUCIBLE;
    img.Init(r.scene.camera.imgWidth, r.scene.camera.imgHeight);
    img.EnableLinear();
    img.EnableFeatures();
    img.EnableToneMap();
    if (img.DepthOfField(lens) || img.DepthOfFieldError().empty()) { fprintf(stderr, "DepthOfField() worked without EnableDepthOfField()\n"); return 7; }
    rt_dof_params dp;
    rt_dof_default_params(&dp);
    dp.max_coc = atoi(argv[7]);
    img.EnableDepthOfField(&dp);
    if (!r.BeginRender()) { fprintf(stderr, "BeginRender failed: %s\n", r.LastError().c_str()); return 4; }
    if (!r.WaitRender()) { fprintf(stderr, "render failed: %s\n", r.LastError().c_str()); return 4; }
    if (!img.Denoise()) { fprintf(stderr, "Denoise failed: %s\n", img.DenoiseError().c_str()); return 8; }
    if (!img.DepthOfField(lens) || !img.GetDefocused() || !img.GetCoc()) { fprintf(stderr, "DepthOfField failed: %s\n", img.DepthOfFieldError().c_str()); return 8; }
    if (!img.ToneMap() || !img.GetDisplayImage()) { fprintf(stderr, "ToneMap failed: %s\n", img.ToneMapError().c_str()); return 8; }
    if (!img.SaveDenoisedImage((prefix + "_den.pfm").c_str()) || !img.SaveDefocusedImage((prefix + "_dof.pfm").c_str()) ||
        !rt::WritePFM((prefix + "_coc.pfm").c_str(), img.GetCoc(), img.GetWidth(), img.GetHeight(), 1)) {
        fprintf(stderr, "saving failed\n");
        return 9;
    }
    // a new upstream plane discards the defocused one
    if (!img.Denoise() || img.GetDefocused()) { fprintf(stderr, "the defocused plane outlived a new Denoise()\n"); return 9; }
    printf("pixels %d of %d\n", img.GetNumRenderedPixels(), img.GetWidth() * img.GetHeight());
    return 0;
}
