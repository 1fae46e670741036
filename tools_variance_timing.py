#!/usr/bin/env python3
"""Measures what the variance plane and the variance-guided denoise cost, and writes one JSON document.
  frames:  the Cornell frame (1920x1080, 64 spp, 1 M generated photons) rendered device-side, synchronously with statistics,
           `--frames` times without the plane and `--frames` times with it, alternating; per frame the wall time of the call on
           its stream (rt_stats.ms_total) and the summed k_resolve intervals (rt_stats.ms_resolve); median, min and max of each.
  denoise: one rt_denoise_device call against one rt_denoise_var_device call on device-resident 1920x1080 planes, five levels,
           HIP events on the call's stream, as tools_denoise_timing.py times it.
--root names the tree to import raytracing_folder_amd from, so that the same script times another checkout (the parent commit,
built, with --no-variance: only the frame without the plane).  profiles/variance_timing.json is assembled from such runs of
one session.
usage: python tools_variance_timing.py [--root DIR] [--no-variance] [--frames 10] [--no-denoise] [--out FILE]"""
import argparse
import os
import sys

from tools_timing import add_common_args, emit, event_times, spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--no-variance", action="store_true")
    ap.add_argument("--no-denoise", action="store_true")
    ap.add_argument("--frames", type=int, default=10)
    add_common_args(ap, calls=None)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--photons", type=int, default=1000000)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np
    import torch
    from raytracing_folder_amd import capi, workloads
    if capi.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing is measured (there is no CPU path)")
    w, h = a.width, a.height
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    res = dict(what="tools_variance_timing.py", root=os.path.basename(os.path.abspath(a.root)), width=w, height=h, spp=a.spp, photons=a.photons)

    s, cam = workloads.load_cornell(w, h)
    s.generate_photons(a.photons, 8, seed=20171203, device=0)
    p = capi.default_params(min_sample=a.spp, max_sample=a.spp, threshold=-1.0)
    tiles = capi.TileRange(32, 8, 0, 1)
    rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device=dev)
    z = torch.zeros((h, w), dtype=torch.float32, device=dev)
    cnt = torch.zeros((h, w), dtype=torch.uint8, device=dev)
    var = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def frame(with_plane):
        if with_plane:
            return s.render_tiles_outputs_device(cam, p, tiles, 0, rgb.data_ptr(), z.data_ptr(), cnt.data_ptr(), stream=stream.cuda_stream,
                                                 sync=True, want_stats=True, variance_ptr=var.data_ptr())
        return s.render_tiles_device(cam, p, tiles, 0, rgb.data_ptr(), z.data_ptr(), cnt.data_ptr(), stream=stream.cuda_stream, sync=True,
                                     want_stats=True)

    kinds = [False] if a.no_variance else [False, True]
    for k in kinds:                                             # warm-up: allocations, queue sizes from measurement
        frame(k), frame(k)
    total, resolve = {k: [] for k in kinds}, {k: [] for k in kinds}
    for _ in range(a.frames):
        for k in kinds:
            st = frame(k)
            total[k].append(st.ms_total), resolve[k].append(st.ms_resolve)
    res["frame_ms"] = {("with_plane" if k else "without_plane"): spread(total[k]) for k in kinds}
    res["resolve_ms"] = {("with_plane" if k else "without_plane"): spread(resolve[k]) for k in kinds}
    res["streams"] = int(st.streams)
    if not a.no_variance:
        v = var.cpu().numpy()
        res["variance_plane"] = dict(finite=bool(np.isfinite(v).all()), mean=float(v.mean()), max=float(v.max()))

    if not a.no_denoise:
        rng = np.random.default_rng(0)
        Y, X = np.mgrid[0:h, 0:w]
        ids = (X * 3 // w).astype(np.int32)
        ids[: h // 10] = -1
        zz = (5.0 + 4.0 * X / w + 2.0 * Y / h).astype(np.float32)
        zz[ids < 0] = 1e30
        normal = np.zeros((h, w, 3), np.float32)
        normal[..., 2] = 1
        normal[Y > h // 2] = (0, 1, 0)
        albedo = np.float32([[0.8, 0.5, 0.3], [0.2, 0.6, 0.9], [0.7, 0.7, 0.7]])[np.clip(ids, 0, 2)]
        clean = albedo * (0.6 + 0.3 * np.sin(X / 50.0) * np.cos(Y / 70.0))[..., None]
        lin = (clean * (1 + 0.3 * rng.normal(0, 1, (h, w, 3)))).astype(np.float32)
        pl = dict(linear=lin, normal=normal, albedo=albedo, z=zz, object_id=ids, variance=((0.3 * clean) ** 2).astype(np.float32))
        t = {k: torch.from_numpy(v).to(dev) for k, v in pl.items()}
        out = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
        out_var = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()

        def call(guided):
            extra = dict(variance_ptr=t["variance"].data_ptr(), out_variance_ptr=out_var.data_ptr()) if guided else {}
            capi.denoise_device(0, stream.cuda_stream, w, h, linear_ptr=t["linear"].data_ptr(), normal_ptr=t["normal"].data_ptr(),
                                albedo_ptr=t["albedo"].data_ptr(), z_ptr=t["z"].data_ptr(), out_ptr=out.data_ptr(),
                                object_id_ptr=t["object_id"].data_ptr(), sync=False, levels=5, **extra)

        res["denoise_ms"] = {}
        for guided in kinds:                                    # one kind after the other, not interleaved
            name = "guided" if guided else "fixed_sigma"
            res["denoise_ms"][name] = spread(event_times(stream, {name: lambda: call(guided)}, 50)[name])
    emit(res, a.out)


if __name__ == "__main__":
    main()
