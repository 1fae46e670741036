#!/usr/bin/env python3
"""Measures what one bloom call costs, and writes one JSON document.
  One rt_bloom_device call on device-resident 1920x1080 planes (linear in, bloomed out, six levels, threshold 0.5 so that the
  frame has pixels above it), HIP events on the call's stream around each call, `--calls` calls after 10 of warm-up; median, min
  and max, for a 1 spp render of the Cornell scene (the linear plane of Scene.render_outputs), and interleaved with it
    in_place   the same call with out == linear
    tiny       a call on a 1 x 1 frame of another rt_bloom: two launches (prefilter, combine), no pixels
  The launches a call makes and the level the tail kernel starts at are printed beside it (rt_bloom_plan), with the bytes the
  definition moves: the frame read twice and written once, every level written and read on the way down and again on the way up.
  --libs name=path,...: the same measurement once per library, each in a child process with RT_MI355X_LIB set -- the shipped
  build (every level a launch of its own), raytracing_folder_amd/lib/variants/librt_bloom_tail.so (`make bloom_tail`: the tail
  kernel within 64 KB of LDS) or a `make variant NAME=tail156k DEFS="-DRT_BLOOM_TAIL=1 -DRT_BLOOM_TAIL_TEXELS=13312"`.
  --trace-calls N (with --libs): per library a second child, run under `rocprofv3 --kernel-trace` with N calls, whose trace gives
  every kernel's own duration -- "kernel_trace_us": per kernel the median over its full-frame dispatches and their number per call.
usage: python tools_bloom_timing.py [--calls 200] [--libs a=path,b=path] [--trace-calls 50] [--out profiles/bloom_timing.json]"""
import argparse
import statistics

from tools_timing import add_common_args, emit, event_times, kernel_durations_us, kernel_trace_db, per_library, repo_on_path, spread


def pyramid_bytes(w, h, levels):
    """(bytes of the full-resolution passes, bytes of the pyramid traffic) of one call by the definition"""
    sizes = [((w + 1) // 2, (h + 1) // 2)]
    while len(sizes) < levels and sizes[-1] != (1, 1):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    texels = [a * b for a, b in sizes]
    # down: every level written once, every level but the last read once.  up: every level but the last read and written once,
    # every level but the first read once; the combine reads level 0
    pyr = 12 * (sum(texels) + sum(texels[:-1]) + 2 * sum(texels[:-1]) + sum(texels[1:]) + texels[0])
    return 12 * w * h * 3, pyr


def measure(a):
    repo_on_path()
    import torch
    from raytracing_folder_amd import capi, workloads
    if capi.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing is measured (there is no CPU path)")
    w, h = a.width, a.height
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    s, cam = workloads.load_cornell(w, h)
    out = s.render_outputs(cam, capi.default_params(shade_model=capi.SHADE_P13, bounce=4, photon_count=0, min_sample=1, max_sample=1, threshold=1e30),
                           planes=("linear",))
    lin = torch.from_numpy(out["linear"]).to(dev)
    dst, work = torch.zeros_like(lin), lin.clone()
    one = torch.full((1, 1, 3), 2.0, dtype=torch.float32, device=dev)
    one_out = torch.zeros_like(one)
    torch.cuda.synchronize()
    kw = dict(threshold=0.5, levels=a.levels)
    with capi.Bloom(0, w, h) as bl, capi.Bloom(0, 1, 1) as tiny:
        calls = dict(
            bloom=lambda: bl.apply_device(stream.cuda_stream, linear_ptr=lin.data_ptr(), out_ptr=dst.data_ptr(), **kw),
            in_place=lambda: bl.apply_device(stream.cuda_stream, linear_ptr=work.data_ptr(), out_ptr=work.data_ptr(), intensity=0.0, **kw),
            tiny=lambda: tiny.apply_device(stream.cuda_stream, linear_ptr=one.data_ptr(), out_ptr=one_out.data_ptr(), **kw))
        res = {k: spread(v) for k, v in event_times(stream, calls, a.calls).items()}
    used, tail = capi.bloom_plan(w, h, a.levels)
    launches = (2 + tail + 1 + tail) if tail >= 0 else 2 + 2 * (used - 1)
    full, pyr = pyramid_bytes(w, h, a.levels)
    floor_us = (full + pyr) / a.peak_gbs / 1e3
    res.update(levels_used=used, tail_level=tail, launches_per_call=launches, bytes_full_resolution=full, bytes_pyramid=pyr,
               byte_floor_us=round(floor_us, 2), peak_gbs=a.peak_gbs,
               fraction_of_peak=round(floor_us / (res["bloom"]["median"] * 1e3), 4),
               bright_fraction=round(float((out["linear"].max(axis=2) > 0.5).mean()), 4))
    return dict(width=w, height=h, **res)


KERNELS = ("k_bloom_prefilter", "k_bloom_down", "k_bloom_tail", "k_bloom_up", "k_bloom_combine")


def kernel_trace(a, env):
    """one child under rocprofv3 --kernel-trace: {kernel: median us over the dispatches of the full frame, dispatches per call}.
    The 1 x 1 calls are one workgroup per kernel; the full frame's prefilter and combine are told from them by their grid, and
    the 1 x 1 frame has no other kernel."""
    child = ["--calls", a.trace_calls, "--width", a.width, "--height", a.height, "--levels", a.levels]
    with kernel_trace_db(__file__, child, env, prefix="bloom_trace_") as db:
        out, total = {}, 0.0
        calls = 2 * (a.trace_calls + 10) + 0.0                  # bloom and in_place, warm-up included
        for k in KERNELS:
            t = kernel_durations_us(db, k, " and grid_x > 256" if k in ("k_bloom_prefilter", "k_bloom_combine") else "")
            if t:
                per_call = len(t) / calls
                out[k] = dict(median_us=round(statistics.median(t), 2), per_call=round(per_call, 2), sum_us_per_call=round(sum(t) / calls, 2))
                total += sum(t) / calls
        out["kernels_sum_us_per_call"] = round(total, 2)
    return dict(command="rocprofv3 --kernel-trace -d DIR -o trace -- python tools_bloom_timing.py --calls %d" % a.trace_calls, **out)


def main():
    ap = argparse.ArgumentParser()
    add_common_args(ap)
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--peak-gbs", type=float, default=8685.0, help="the streaming peak the byte floor is set against (profiles/r04_peaks.json)")
    ap.add_argument("--libs", default=None, help="name=path,...: measure each library in a child process")
    ap.add_argument("--trace-calls", type=int, default=0, help="(--libs) calls of the extra child run under rocprofv3 --kernel-trace; 0: none")
    a = ap.parse_args()
    if a.libs:
        child = ["--calls", a.calls, "--width", a.width, "--height", a.height, "--levels", a.levels, "--peak-gbs", a.peak_gbs]
        trace = (lambda name, env, doc: doc.update(kernel_trace_us=kernel_trace(a, env))) if a.trace_calls else None
        res = dict(what="tools_bloom_timing.py", libraries=per_library(__file__, a.libs, child, trace))
    else:
        res = dict(what="tools_bloom_timing.py", **measure(a))
    emit(res, a.out)


if __name__ == "__main__":
    main()
