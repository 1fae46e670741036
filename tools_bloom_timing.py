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
import json
import os
import shutil
import sqlite3
import statistics
import subprocess
import sys
import tempfile


def spread(ms):
    ms = sorted(ms)
    return dict(median=round(statistics.median(ms), 4), min=round(ms[0], 4), max=round(ms[-1], 4), n=len(ms))


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
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
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
        ms = {k: [] for k in calls}
        with torch.cuda.stream(stream):
            for _ in range(10):
                for c in calls.values():
                    c()
            stream.synchronize()
            for _ in range(a.calls):
                for k, c in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    c()
                    e1.record(stream)
                    e1.synchronize()
                    ms[k].append(e0.elapsed_time(e1))
        res = {k: spread(v) for k, v in ms.items()}
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
    tmp = tempfile.mkdtemp(prefix="bloom_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "-d", tmp, "-o", "trace", "--", sys.executable, os.path.abspath(__file__), "--calls", str(a.trace_calls),
           "--width", str(a.width), "--height", str(a.height), "--levels", str(a.levels)]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit(f"kernel trace: exit {r.returncode}\n{r.stdout}\n{r.stderr}")
        dbs = [os.path.join(d, f) for d, _, fs in os.walk(tmp) for f in fs if f.endswith(".db")]
        if not dbs:
            raise SystemExit("kernel trace: rocprofv3 left no database")
        db = sqlite3.connect(dbs[0])
        out, total = {}, 0.0
        calls = 2 * (a.trace_calls + 10) + 0.0                  # bloom and in_place, warm-up included
        for k in KERNELS:
            full = " and grid_x > 256" if k in ("k_bloom_prefilter", "k_bloom_combine") else ""
            t = [row[0] / 1000.0 for row in db.execute(f"select end - start from kernels where name like '%{k}%'{full} order by start")]
            if t:
                per_call = len(t) / calls
                out[k] = dict(median_us=round(statistics.median(t), 2), per_call=round(per_call, 2), sum_us_per_call=round(sum(t) / calls, 2))
                total += sum(t) / calls
        out["kernels_sum_us_per_call"] = round(total, 2)
        db.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return dict(command="rocprofv3 --kernel-trace -d DIR -o trace -- python tools_bloom_timing.py --calls %d" % a.trace_calls, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--peak-gbs", type=float, default=8685.0, help="the streaming peak the byte floor is set against (profiles/r04_peaks.json)")
    ap.add_argument("--libs", default=None, help="name=path,...: measure each library in a child process")
    ap.add_argument("--trace-calls", type=int, default=0, help="(--libs) calls of the extra child run under rocprofv3 --kernel-trace; 0: none")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.libs:
        res = dict(what="tools_bloom_timing.py", libraries={})
        for item in a.libs.split(","):
            name, path = item.split("=", 1)
            env = dict(os.environ, RT_MI355X_LIB=os.path.abspath(path))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--calls", str(a.calls), "--width", str(a.width), "--height", str(a.height),
                                "--levels", str(a.levels), "--peak-gbs", str(a.peak_gbs)], env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:       # a child that died says why, and nothing more is started on the device
                raise SystemExit(f"{name}: exit {r.returncode}\n{r.stdout}\n{r.stderr}")
            res["libraries"][name] = json.loads(r.stdout.strip().splitlines()[-1])
            if a.trace_calls:
                res["libraries"][name]["kernel_trace_us"] = kernel_trace(a, env)
    else:
        res = dict(what="tools_bloom_timing.py", **measure(a))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
