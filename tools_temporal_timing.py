#!/usr/bin/env python3
"""Measures what one temporal accumulation costs and what it buys, and writes one JSON document.
  accumulate: one rt_temporal_device call on device-resident 1920x1080 planes with a history that holds a frame, the camera
              alternating between two positions 0.3 apart (every call reprojects and gathers), with and without the variance
              plane, the two alternating; HIP events on the call's stream around each call, `--calls` calls after 10 of warm-up;
              median, min and max.  Bytes: what a pixel moves (inputs, outputs, the history records written and the four taps'
              records read, counted once each as if no tap were shared), so that the time can be set beside the memory rate.
  quality:    cornell_gi.xml (live GI) at 96x72, reproducible mode: eight 4 spp frames (seeds 1..8) through
              Scene.render_temporal against a 64 spp frame of another seed -- linear RMSE over hit pixels of frame 8 alone, of the
              accumulated frame and of the variance-guided denoise on top, for a fixed camera and for one translated by 0.3 (1 %
              of the scene's width) between frames.
usage: python tools_temporal_timing.py [--calls 200] [--no-quality] [--out profiles/temporal_timing.json]"""
import argparse

from tools_timing import add_common_args, emit, event_times, repo_on_path, spread


def quality(capi, workloads, np):
    common = dict(shade_model=capi.SHADE_P12, bounce=8, hemisphere_sample=1, photon_count=0)
    noisy = lambda seed: capi.default_params(min_sample=4, max_sample=8, threshold=1e30, seed=seed, **common)
    target = capi.default_params(min_sample=64, max_sample=64, threshold=-1.0, seed=77, **common)
    res = {}
    for name, step in (("fixed_camera", 0.0), ("camera_moving_0.3_a_frame", 0.3)):
        s, cam = workloads.load_cornell_gi(96, 72)
        s.set_render_flags(capi.RENDER_REPRODUCIBLE)
        with capi.History(0, 96, 72) as hst:
            for seed in range(1, 9):
                out = s.render_temporal(hst, cam, noisy(seed))
                if seed < 8:
                    cam.pos[0] += step
        ref = s.render_outputs(cam, target, planes=("linear", "object_id"))
        valid = (out["object_id"] >= 0) & (ref["object_id"] >= 0)
        rmse = lambda a: float(np.sqrt(((a[valid].astype(np.float64) - ref["linear"][valid]) ** 2).mean()))
        one, acc, den = rmse(out["linear"]), rmse(out["accumulated"]), rmse(out["denoised"])
        res[name] = dict(rmse_4spp=round(one, 6), rmse_accumulated=round(acc, 6), rmse_denoised_on_top=round(den, 6),
                         ratio_accumulated=round(acc / one, 4), ratio_denoised_on_top=round(den / one, 4),
                         mean_history=round(float(out["history"][out["object_id"] >= 0].mean()), 3))
    return res


def main():
    ap = argparse.ArgumentParser()
    add_common_args(ap)
    ap.add_argument("--no-quality", action="store_true")
    a = ap.parse_args()
    repo_on_path()
    import numpy as np
    import torch
    from raytracing_folder_amd import capi, workloads
    if capi.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing is measured (there is no CPU path)")
    w, h = a.width, a.height
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    res = dict(what="tools_temporal_timing.py", width=w, height=h)

    # a wall 10 away seen from two camera positions: every pixel has a history, its taps lie a few pixels from it
    cams = []
    for x in (0.0, 0.3):
        cam = capi.Camera()
        cam.pos[:], cam.dir[:], cam.up[:] = (x, 0.0, 10.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0)
        cam.fov, cam.focaldist, cam.dof, cam.width, cam.height = 40.0, 1.0, 0.0, w, h
        cams.append(cam)
    rng = np.random.default_rng(0)
    Y, X = np.mgrid[0:h, 0:w]
    half_h = 10 * np.tan(np.radians(20.0))
    px, py = (X + 0.5 - w / 2) * (2 * half_h / h), -(Y + 0.5 - h / 2) * (2 * half_h / h)
    z = np.sqrt(px * px + py * py + 100.0).astype(np.float32)
    ids = (X * 3 // w).astype(np.int32)
    normal = np.zeros((h, w, 3), np.float32)
    normal[..., 2] = 1
    albedo = np.float32([[0.8, 0.5, 0.3], [0.2, 0.6, 0.9], [0.7, 0.7, 0.7]])[ids]
    clean = albedo * (0.6 + 0.3 * np.sin(X / 50.0) * np.cos(Y / 70.0))[..., None]
    lin = (clean * (1 + 0.3 * rng.normal(0, 1, (h, w, 3)))).astype(np.float32)
    pl = dict(linear=lin, normal=normal, albedo=albedo, z=z, object_id=np.zeros((h, w), np.int32), variance=((0.3 * clean) ** 2).astype(np.float32))
    t = {k: torch.from_numpy(v).to(dev) for k, v in pl.items()}
    out, out_var, hist = (torch.zeros((h, w, 3), dtype=torch.float32, device=dev), torch.zeros((h, w, 3), dtype=torch.float32, device=dev),
                          torch.zeros((h, w), dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    histories = {False: capi.History(0, w, h), True: capi.History(0, w, h)}
    count = {False: 0, True: 0}

    def call(with_var):
        extra = dict(variance_ptr=t["variance"].data_ptr(), out_variance_ptr=out_var.data_ptr()) if with_var else {}
        count[with_var] += 1
        histories[with_var].accumulate_device(stream.cuda_stream, cams[count[with_var] & 1], linear_ptr=t["linear"].data_ptr(),
                                              normal_ptr=t["normal"].data_ptr(), albedo_ptr=t["albedo"].data_ptr(), z_ptr=t["z"].data_ptr(),
                                              object_id_ptr=t["object_id"].data_ptr(), out_ptr=out.data_ptr(), history_ptr=hist.data_ptr(),
                                              sync=False, **extra)

    ms = event_times(stream, {False: lambda: call(False), True: lambda: call(True)}, a.calls)
    res["accumulate_ms"] = {("with_variance" if k else "without_variance"): spread(v) for k, v in ms.items()}
    res["mean_history"] = float(hist.mean().item())
    # per pixel: rgb, normal, albedo 12 each, z 4, id 4 (+ variance 12) in; linear 12, history 4 (+ variance 12) out; 48 of records
    # written; four taps of 48
    res["bytes_per_pixel"] = dict(without_variance=12 * 3 + 8 + 16 + 48 + 4 * 48, with_variance=12 * 3 + 8 + 16 + 24 + 48 + 4 * 48)
    for k in histories.values():
        k.close()
    if not a.no_quality:
        res["quality_cornell_gi_96x72"] = quality(capi, workloads, np)
    emit(res, a.out)


if __name__ == "__main__":
    main()
