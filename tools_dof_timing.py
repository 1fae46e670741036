#!/usr/bin/env python3
"""Measures what one depth-of-field call costs, and writes one JSON document.
  One rt_dof_device call on device-resident 1920x1080 planes (linear and z in, defocused out; the default parameters: K = 16,
  N = 32), HIP events on the call's stream around each call, `--calls` calls after 10 of warm-up; median, min and max, for three
  synthetic frames, interleaved:
    sharp      dof = 0: every tile takes the early out
    third      the lower third of the frame lies far beyond the focus (|c| = K there), the rest is in focus
    all        every pixel at |c| >= K: no early out anywhere, every tap is taken
  Beside each: the bytes the definition moves at the least (k_dof_coc reads z, 4 B a pixel, and writes (c, D), 8 B; the gather
  reads the colour, 12 B, and writes it, 12 B; where a pixel is gathered also its own (c, D), 8 B -- the taps are taken as cache
  hits) and what fraction of `--peak-gbs` that is at the measured time.  "early_out_floor": the 12 B in, 12 B out and 8 B of
  (c, D) a pixel that a frame in focus cannot avoid.
  --trace-calls N: per frame one child process, run under `rocprofv3 --kernel-trace` with N calls of that frame alone, whose trace
  gives every kernel's own duration -- "kernel_trace_us": per kernel the median over its dispatches.
  --lens: also the comparison with the renderer's own lens (cornell.xml 96 x 72 at 256 spp, focused on the teapot): RMSE in linear
  colour against a lens render of a second lens render (e_noise), the pinhole render (e_pin) and the stage on the pinhole render
  (e_post).
usage: python tools_dof_timing.py [--calls 200] [--trace-calls 50] [--lens] [--out profiles/dof_timing.json]"""
import argparse
import math
import statistics

from tools_timing import add_common_args, emit, event_times, kernel_durations_us, kernel_trace_db, repo_on_path, spread

FRAMES = ("sharp", "third", "all")
KERNELS = ("k_dof_coc", "k_dof_neighbour_max", "k_dof_gather")
FOCUS, FOV = 10.0, 40.0


def make_frame(kind, w, h, K):
    """(linear, z, the camera's dof) as numpy arrays and a float: A = K pixels except for `sharp`"""
    import numpy as np
    rng = np.random.default_rng(1)
    lin = (2.0 ** rng.uniform(-4.0, 4.0, (h, w, 1)) * rng.uniform(0.5, 1.5, (h, w, 3))).astype(np.float32)
    Y, X = np.mgrid[0:h, 0:w]
    t = math.tan(math.radians(FOV / 2))                         # the plane in focus: axial depth FOCUS, z along the pixel's ray
    tx, ty = ((X + 0.5) / w - 0.5) * 2.0 * t * w / h, ((Y + 0.5) / h - 0.5) * 2.0 * t
    z = (FOCUS * np.sqrt(1.0 + tx * tx + ty * ty)).astype(np.float32)
    if kind == "third":
        z[Y >= 2 * h // 3] = 1e30
    elif kind == "all":
        z[:] = 1e30
    dof = 0.0 if kind == "sharp" else K * 2.0 * FOCUS * math.tan(math.radians(FOV / 2)) / h
    return lin, z, dof


def gathered_fraction(tiles, w, h, K):
    """the fraction of pixels whose R (the stage's own out_tiles) is half a pixel or more"""
    import numpy as np
    Y, X = np.mgrid[0:h, 0:w]
    return float((tiles[Y // K, X // K] >= 0.5).mean())


def measure(a):
    repo_on_path()
    import torch
    from raytracing_folder_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing is measured (there is no CPU path)")
    w, h = a.width, a.height
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    kw = dict(max_coc=a.max_coc, samples=a.samples)
    kinds = [a.frame] if a.frame else list(FRAMES)
    tx, ty = capi.dof_tiles(w, h, a.max_coc)
    planes, cams, info = {}, {}, {}
    for kind in kinds:
        lin, z, dof = make_frame(kind, w, h, a.max_coc)
        planes[kind] = [torch.from_numpy(x).to(dev) for x in (lin, z)] + [torch.zeros((h, w, 3), dtype=torch.float32, device=dev)]
        cam = capi.Camera()
        cam.dir[:], cam.up[:] = (0, 1, 0), (0, 0, 1)
        cam.fov, cam.focaldist, cam.dof, cam.width, cam.height = FOV, FOCUS, dof, w, h
        cams[kind] = cam
    torch.cuda.synchronize()
    with capi.DepthOfField(0, w, h) as d:
        tiles = torch.zeros((ty, tx), dtype=torch.float32, device=dev)
        for kind, p in planes.items():                          # what fraction is gathered: from the stage's own R
            d.apply_device(stream.cuda_stream, cams[kind], linear_ptr=p[0].data_ptr(), z_ptr=p[1].data_ptr(), out_ptr=p[2].data_ptr(),
                           tiles_ptr=tiles.data_ptr(), sync=True, **kw)
            info[kind] = dict(camera_dof=round(cams[kind].dof, 6), gathered=round(gathered_fraction(tiles.cpu().numpy(), w, h, a.max_coc), 4))
        calls = {kind: (lambda p=p, c=cams[kind]: d.apply_device(stream.cuda_stream, c, linear_ptr=p[0].data_ptr(), z_ptr=p[1].data_ptr(),
                                                                 out_ptr=p[2].data_ptr(), **kw)) for kind, p in planes.items()}
        ms = event_times(stream, calls, a.calls)
    res = {}
    n = w * h
    for kind in kinds:
        least = n * (4 + 8 + 12 + 12) + int(info[kind]["gathered"] * n) * 8
        t = spread(ms[kind])
        floor_us = least / a.peak_gbs / 1e3
        res[kind] = dict(call_ms=t, bytes_least=least, byte_floor_us=round(floor_us, 2), gbs_at_median=round(least / (t["median"] * 1e6), 1),
                         fraction_of_peak=round(floor_us / (t["median"] * 1e3), 4), **info[kind])
    early = n * (12 + 12 + 8)
    return dict(width=w, height=h, peak_gbs=a.peak_gbs, launches_per_call=3, frames=res,
                early_out_floor=dict(bytes=early, us=round(early / a.peak_gbs / 1e3, 2)), **kw)


def lens(w=96, h=72, spp=256, focus=65.0, dof=3.0):
    """the stage against the renderer's own lens on cornell.xml: RMSEs in linear colour over the pixels finite in all four"""
    repo_on_path()
    import numpy as np
    from raytracing_folder_amd import capi, workloads
    s, cam = workloads.load_cornell(w, h)
    cam.focaldist, cam.dof = focus, dof
    s.set_render_flags(capi.RENDER_REPRODUCIBLE)                # the same figures on every run
    pin = capi._copy_camera(cam)
    pin.dof = 0.0
    par = lambda seed: capi.default_params(shade_model=capi.SHADE_P13, bounce=6, photon_count=0, threshold=1e-3, seed=seed, min_sample=spp, max_sample=spp)
    L1 = s.render_outputs(cam, par(21), planes=("linear",))["linear"]
    L2 = s.render_outputs(cam, par(22), planes=("linear",))["linear"]
    P = s.render_outputs(pin, par(21), planes=("linear",))
    with capi.DepthOfField(0, w, h) as d:
        S, coc = d.apply(P["linear"], P["z"], cam, return_coc=True)
    ok = np.isfinite(L1).all(axis=2) & np.isfinite(L2).all(axis=2) & np.isfinite(P["linear"]).all(axis=2) & np.isfinite(S).all(axis=2)
    rmse = lambda a, b: float(np.sqrt(np.mean((a[ok].astype(np.float64) - b[ok].astype(np.float64)) ** 2)))
    e_noise, e_pin, e_post = rmse(L1, L2), rmse(P["linear"], L1), rmse(S, L1)
    return dict(scene="cornell.xml", width=w, height=h, spp=spp, focaldist=focus, dof=dof, A_px=round(dof * h / (2.0 * focus * math.tan(math.radians(cam.fov / 2))), 3),
                coc_min=round(float(coc.min()), 3), coc_max=round(float(coc.max()), 3),
                e_noise=round(e_noise, 6), e_pin=round(e_pin, 6), e_post=round(e_post, 6),
                e_post_over_e_pin=round(e_post / e_pin, 4), e_noise_over_e_pin=round(e_noise / e_pin, 4))


def kernel_trace(a, kind):
    """one child under rocprofv3 --kernel-trace running `kind` alone: {kernel: median us over its dispatches}"""
    child = ["--calls", a.trace_calls, "--width", a.width, "--height", a.height, "--max-coc", a.max_coc, "--samples", a.samples, "--frame", kind]
    with kernel_trace_db(__file__, child, prefix="dof_trace_") as db:
        out, total = {}, 0.0
        for k in KERNELS:
            t = kernel_durations_us(db, k)
            if t:
                out[k] = dict(median_us=round(statistics.median(t), 2), min_us=round(min(t), 2), dispatches=len(t))
                total += statistics.median(t)
        out["kernels_sum_us_per_call"] = round(total, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    add_common_args(ap)
    ap.add_argument("--max-coc", type=int, default=16)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--lens", action="store_true", help="also compare the stage with the renderer's own lens render")
    ap.add_argument("--frame", default=None, choices=FRAMES, help="measure this frame alone (what the trace children do)")
    ap.add_argument("--peak-gbs", type=float, default=8685.0, help="the streaming peak the byte floor is set against (profiles/r04_peaks.json)")
    ap.add_argument("--trace-calls", type=int, default=0, help="calls of the extra children run under rocprofv3 --kernel-trace; 0: none")
    a = ap.parse_args()
    res = dict(what="tools_dof_timing.py", **measure(a))
    if a.trace_calls and not a.frame:
        res["kernel_trace_command"] = "rocprofv3 --kernel-trace -d DIR -o trace -- python tools_dof_timing.py --calls %d --frame FRAME" % a.trace_calls
        for kind in FRAMES:
            res["frames"][kind]["kernel_trace_us"] = kernel_trace(a, kind)
    if a.lens and not a.frame:
        res["lens"] = lens()
    emit(res, a.out)


if __name__ == "__main__":
    main()
