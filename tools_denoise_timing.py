#!/usr/bin/env python3
"""Measures one rt_denoise_device call on device-resident planes and writes profiles/denoise_timing.json.
The planes are synthetic (a smooth frame with three objects, a background band and 30 % multiplicative noise); the call is
timed with HIP events on the stream it is enqueued on: warm-up calls first, then `--repeat` calls timed one by one, median
and spread reported.  Next to the time: the bytes the taps of one level request (25 taps x two 16-byte records per pixel)
and the rate that implies, for comparison with the measured ceilings of profiles/r04_peaks.json.
usage: python tools_denoise_timing.py [--width 1920 --height 1080 --levels 5 --warmup 10 --repeat 50 --no-ids --rgb8]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from raytracing_folder_amd import capi
from tools_timing import emit, event_times


def planes(w, h, seed=0):
    rng = np.random.default_rng(seed)
    Y, X = np.mgrid[0:h, 0:w]
    ids = (X * 3 // w).astype(np.int32)
    ids[: h // 10] = -1
    z = (5.0 + 4.0 * X / w + 2.0 * Y / h).astype(np.float32)
    z[ids < 0] = 1e30
    normal = np.zeros((h, w, 3), np.float32)
    normal[..., 2] = 1
    normal[Y > h // 2] = (0, 1, 0)
    albedo = np.float32([[0.8, 0.5, 0.3], [0.2, 0.6, 0.9], [0.7, 0.7, 0.7]])[np.clip(ids, 0, 2)]
    light = (0.6 + 0.3 * np.sin(X / 50.0) * np.cos(Y / 70.0))[..., None]
    lin = (albedo * light * (1 + 0.3 * rng.normal(0, 1, (h, w, 3)))).astype(np.float32)
    return dict(linear=lin, normal=normal, albedo=albedo, z=z, object_id=ids)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=50)
    ap.add_argument("--no-ids", action="store_true")
    ap.add_argument("--rgb8", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_timing.json"))
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing is measured (there is no CPU path)")
    w, h = a.width, a.height
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(v).to(dev) for k, v in planes(w, h).items()}
    out = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    out8 = torch.zeros((h, w, 3), dtype=torch.uint8, device=dev) if a.rgb8 else None
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def call():
        capi.denoise_device(0, stream.cuda_stream, w, h, linear_ptr=t["linear"].data_ptr(), normal_ptr=t["normal"].data_ptr(),
                            albedo_ptr=t["albedo"].data_ptr(), z_ptr=t["z"].data_ptr(), out_ptr=out.data_ptr(),
                            object_id_ptr=None if a.no_ids else t["object_id"].data_ptr(),
                            rgb8_ptr=out8.data_ptr() if a.rgb8 else None, sync=False, levels=a.levels)

    ms = sorted(event_times(stream, dict(call=call), a.repeat, warmup=a.warmup)["call"])
    med = statistics.median(ms)
    level_bytes = 25 * 32 * w * h                               # requested by the taps of one level (served mostly from cache)
    unique_bytes = (32 + 16) * w * h                            # what a level must move at least: read both records once, write one
    peaks = json.load(open(os.path.join(ROOT, "profiles", "r04_peaks.json")))
    res = dict(what="tools_denoise_timing.py: one rt_denoise_device call, HIP events on the call's stream, device-resident planes",
               width=w, height=h, levels=a.levels, object_id=not a.no_ids, rgb8=a.rgb8, warmup=a.warmup, repeat=a.repeat,
               ms_median=round(med, 4), ms_min=round(ms[0], 4), ms_p90=round(ms[int(0.9 * (len(ms) - 1))], 4), ms_max=round(ms[-1], 4),
               ms_per_level_upper_bound=round(med / a.levels, 4),
               tap_bytes_per_level=level_bytes, unique_bytes_per_level=unique_bytes,
               tap_GBps_at_median=round(a.levels * level_bytes / (med * 1e-3) / 1e9, 1),
               l1_peak_GBps=peaks.get("l1_peak_GBps"), scratch_bytes=48 * w * h)
    emit(res, a.out)


if __name__ == "__main__":
    main()
