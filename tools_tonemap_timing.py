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
import json
import os
import statistics
import shutil
import sqlite3
import subprocess
import sys
import tempfile


def spread(ms):
    ms = sorted(ms)
    return dict(median=round(statistics.median(ms), 4), min=round(ms[0], 4), max=round(ms[-1], 4), n=len(ms))


def measure(a):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
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
    tmp = tempfile.mkdtemp(prefix="tonemap_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "-d", tmp, "-o", "trace", "--", sys.executable, os.path.abspath(__file__), "--calls", str(a.trace_calls),
           "--width", str(a.width), "--height", str(a.height)]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit(f"kernel trace: exit {r.returncode}\n{r.stdout}\n{r.stderr}")
        dbs = [os.path.join(d, f) for d, _, fs in os.walk(tmp) for f in fs if f.endswith(".db")]
        if not dbs:
            raise SystemExit("kernel trace: rocprofv3 left no database")
        db = sqlite3.connect(dbs[0])
        out = {"cornell": {}, "constant": {}}
        for k in KERNELS:
            full = "" if k == "k_exposure_meter" else " and grid_x > 256"
            t = [row[0] / 1000.0 for row in db.execute(f"select end - start from kernels where name like '%{k}%'{full} order by start")]
            half = len(t) // 2
            out["cornell"][k], out["constant"][k] = round(statistics.median(t[:half]), 2), round(statistics.median(t[half:]), 2)
        db.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return dict(command="rocprofv3 --kernel-trace -d DIR -o trace -- python tools_tonemap_timing.py --calls %d" % a.trace_calls, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--libs", default=None, help="name=path,...: measure each library in a child process")
    ap.add_argument("--trace-calls", type=int, default=0, help="(--libs) calls of the extra child run under rocprofv3 --kernel-trace; 0: none")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.libs:
        res = dict(what="tools_tonemap_timing.py", libraries={})
        for item in a.libs.split(","):
            name, path = item.split("=", 1)
            env = dict(os.environ, RT_MI355X_LIB=os.path.abspath(path))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--calls", str(a.calls), "--width", str(a.width), "--height", str(a.height)],
                               env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:       # a child that died says why, and nothing more is started on the device
                raise SystemExit(f"{name}: exit {r.returncode}\n{r.stdout}\n{r.stderr}")
            res["libraries"][name] = json.loads(r.stdout.strip().splitlines()[-1])
            if a.trace_calls:
                res["libraries"][name]["kernel_trace_us"] = kernel_trace(a, env)
    else:
        res = dict(what="tools_tonemap_timing.py", **measure(a))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
