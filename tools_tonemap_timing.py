#!/usr/bin/env python3
"""Measures what one exposure-and-tone-mapping call costs, and writes one JSON document.
  One rt_tonemap_device call on device-resident 1920x1080 planes (linear in, object ids, rgb8 out; ACES), HIP events on the
  call's stream around each call, `--calls` calls after 10 of warm-up; median, min and max, for two frames:
    cornell   a 1 spp render of the Cornell scene (the linear and object-id planes of Scene.render_outputs)
    constant  every pixel (0.5, 0.5, 0.5): one bin, the worst contention a histogram meets
  and per frame three calls, interleaved:
    all            metered: k_luminance_hist, k_exposure_meter, k_tonemap
    tonemap_only   auto_exposure = 0: k_tonemap alone
    fixed          a metered call on a 1 x 1 frame of the same state: three launches and the one-workgroup meter, no pixels
  and all - tonemap_only as hist_and_meter_derived_ms: k_luminance_hist + k_exposure_meter with their two launch gaps (events on
  a stream cannot take the kernels of one call apart; a kernel trace can).
  The bytes a pixel moves are printed beside it (hist: 12 of colour + 4 of id; tonemap: 12 in, 3 out).
  --libs name=path,...: the same measurement once per library, each in a child process with RT_MI355X_LIB set -- the variants of
  `make variant NAME=hist1 DEFS=-DRT_TONEMAP_HIST=1` (rt_tonemap.hip says what 0, 1 and 2 are) and of
  `make variant NAME=blocks256 DEFS=-DRT_TONEMAP_HIST_MAX_BLOCKS=256` (the cap of k_luminance_hist's grid).
  --trace-calls N (with --libs): per library a second child, run under `rocprofv3 --kernel-trace` with N calls, whose trace gives
  every kernel's own duration -- "kernel_trace_us" per frame, the median over the full-frame dispatches, beside the command.
usage: python tools_tonemap_timing.py [--calls 200] [--libs a=path,b=path] [--trace-calls 50] [--out profiles/tonemap_timing.json]"""
import argparse
import statistics

from tools_timing import add_common_args, emit, event_times, kernel_durations_us, kernel_trace_db, per_library, repo_on_path, spread


def measure(a):
    repo_on_path()
    import numpy as np
    import torch
    from raytracing_folder_amd import capi, workloads
    if capi.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing is measured (there is no CPU path)")
    w, h = a.width, a.height
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    s, cam = workloads.load_cornell(w, h)
    out = s.render_outputs(cam, capi.default_params(shade_model=capi.SHADE_P13, bounce=4, photon_count=0, min_sample=1, max_sample=1, threshold=1e30),
                           planes=("linear", "object_id"))
    frames = dict(cornell=(out["linear"], out["object_id"]),
                  constant=(np.full((h, w, 3), 0.5, np.float32), np.zeros((h, w), np.int32)))
    rgb8 = torch.zeros((h, w, 3), dtype=torch.uint8, device=dev)
    one = torch.full((1, 1, 3), 0.5, dtype=torch.float32, device=dev)
    one8 = torch.zeros((1, 1, 3), dtype=torch.uint8, device=dev)
    res = {}
    for name, (lin, ids) in frames.items():
        tl, ti = torch.from_numpy(lin).to(dev), torch.from_numpy(ids).to(dev)
        torch.cuda.synchronize()
        with capi.Exposure(0) as exp:
            calls = dict(
                all=lambda: exp.tonemap_device(stream.cuda_stream, w, h, linear_ptr=tl.data_ptr(), object_id_ptr=ti.data_ptr(), rgb8_ptr=rgb8.data_ptr(), sync=False),
                tonemap_only=lambda: exp.tonemap_device(stream.cuda_stream, w, h, linear_ptr=tl.data_ptr(), rgb8_ptr=rgb8.data_ptr(), sync=False,
                                                        auto_exposure=0, exposure_ev=1.0),
                fixed=lambda: exp.tonemap_device(stream.cuda_stream, 1, 1, linear_ptr=one.data_ptr(), rgb8_ptr=one8.data_ptr(), sync=False))
            ms = event_times(stream, calls, a.calls)
            exp.tonemap_device(stream.cuda_stream, w, h, linear_ptr=tl.data_ptr(), object_id_ptr=ti.data_ptr(), rgb8_ptr=rgb8.data_ptr())
            r = {k: spread(v) for k, v in ms.items()}
            r["hist_and_meter_derived_ms"] = round(r["all"]["median"] - r["tonemap_only"]["median"], 4)
            r["metered_pixels"], r["log2_exposure"] = exp.metered_pixels, round(exp.log2_exposure, 4)
            r["nonempty_bins"] = int((exp.histogram() > 0).sum())
        res[name] = r
    return dict(width=w, height=h, frames=res, bytes_per_pixel=dict(k_luminance_hist=16, k_tonemap_rgb8_only=15))


KERNELS = ("k_luminance_hist", "k_exposure_meter", "k_tonemap")


def kernel_trace(a, env):
    """one child under rocprofv3 --kernel-trace: {frame: {kernel: median us}} from the trace's `kernels` view.  The frames are
    measured one after the other (cornell, constant) with the same number of dispatches, so the dispatches of a kernel on the
    full frame, in start order, fall into halves; the 1 x 1 calls (one workgroup) are left out except for the meter, which is
    always one workgroup."""
    with kernel_trace_db(__file__, ["--calls", a.trace_calls, "--width", a.width, "--height", a.height], env, prefix="tonemap_trace_") as db:
        out = {"cornell": {}, "constant": {}}
        for k in KERNELS:
            t = kernel_durations_us(db, k, "" if k == "k_exposure_meter" else " and grid_x > 256")
            half = len(t) // 2
            out["cornell"][k], out["constant"][k] = round(statistics.median(t[:half]), 2), round(statistics.median(t[half:]), 2)
    return dict(command="rocprofv3 --kernel-trace -d DIR -o trace -- python tools_tonemap_timing.py --calls %d" % a.trace_calls, **out)


def main():
    ap = argparse.ArgumentParser()
    add_common_args(ap)
    ap.add_argument("--libs", default=None, help="name=path,...: measure each library in a child process")
    ap.add_argument("--trace-calls", type=int, default=0, help="(--libs) calls of the extra child run under rocprofv3 --kernel-trace; 0: none")
    a = ap.parse_args()
    if a.libs:
        trace = (lambda name, env, doc: doc.update(kernel_trace_us=kernel_trace(a, env))) if a.trace_calls else None
        res = dict(what="tools_tonemap_timing.py",
                   libraries=per_library(__file__, a.libs, ["--calls", a.calls, "--width", a.width, "--height", a.height], trace))
    else:
        res = dict(what="tools_tonemap_timing.py", **measure(a))
    emit(res, a.out)


if __name__ == "__main__":
    main()
