#!/usr/bin/env python3
"""Measures what one motion blur call costs, and writes one JSON document.
  One rt_motion_blur_device call on device-resident 1920x1080 planes (linear, motion and z in, blurred out; the default parameters:
  K = 16, N = 15), HIP events on the call's stream around each call, `--calls` calls after 10 of warm-up; median, min and max, for
  three synthetic frames, interleaved:
    static     nothing moves: every tile takes the early out
    object     a 256 x 256 square in front of a far background moves with v = (12, 4); the rest is at rest
    all        every pixel moves with |v| = K: no early out anywhere, every tap is taken
  Beside each: the bytes the definition moves at the least (the tile-max pass reads the motion plane, 12 B a pixel; the gather
  reads the colour, 12 B, and writes it, 12 B; where a pixel is gathered also its own motion and z, 16 B -- the taps are taken as
  cache hits) and what fraction of `--peak-gbs` that is at the measured time.
  --trace-calls N: per frame one child process, run under `rocprofv3 --kernel-trace` with N calls of that frame alone, whose trace
  gives every kernel's own duration -- "kernel_trace_us": per kernel the median over its dispatches.
usage: python tools_motion_blur_timing.py [--calls 200] [--trace-calls 50] [--out profiles/motion_blur_timing.json]"""
import argparse
import statistics

from tools_timing import add_common_args, emit, event_times, kernel_durations_us, kernel_trace_db, repo_on_path, spread

FRAMES = ("static", "object", "all")
KERNELS = ("k_mblur_tile_max", "k_mblur_neighbour_max", "k_mblur_gather")


def make_frame(kind, w, h, K, shutter):
    """(linear, motion, z, the fraction of pixels at rest) as numpy arrays"""
    import numpy as np
    rng = np.random.default_rng(1)
    lin = (2.0 ** rng.uniform(-4.0, 4.0, (h, w, 1)) * rng.uniform(0.5, 1.5, (h, w, 3))).astype(np.float32)
    Y, X = np.mgrid[0:h, 0:w]
    z = np.full((h, w), 10.0, np.float32)
    vx, vy = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    if kind == "object":
        sq = (abs(X - w // 2) < 128) & (abs(Y - h // 2) < 128)
        z[sq] = 5.0
        vx[sq], vy[sq] = 12.0, 4.0
    elif kind == "all":
        vx[:] = float(K)
    half = np.float32(0.5 * shutter)
    motion = np.stack([X.astype(np.float32) - vx / half, Y.astype(np.float32) - vy / half, z], axis=2).astype(np.float32)
    return lin, motion, z, float((vx == 0).mean())


def gathered_fraction(motion, K, shutter):
    """the fraction of pixels whose 3 x 3 tile neighbourhood holds a velocity of half a pixel or more"""
    import numpy as np
    h, w = motion.shape[:2]
    Y, X = np.mgrid[0:h, 0:w]
    half = np.float32(0.5 * shutter)
    m = (half * (X - motion[..., 0])) ** 2 + (half * (Y - motion[..., 1])) ** 2
    ty, tx = -(-h // K), -(-w // K)
    pad = np.zeros((ty * K, tx * K))
    pad[:h, :w] = m
    t = pad.reshape(ty, K, tx, K).max(axis=(1, 3))
    big = np.pad(t, 1)
    n = np.max([big[1 + dy:1 + dy + ty, 1 + dx:1 + dx + tx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    return float((n[Y // K, X // K] >= 0.25).mean())


def measure(a):
    repo_on_path()
    import torch
    from raytracing_folder_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing is measured (there is no CPU path)")
    w, h = a.width, a.height
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    kw = dict(max_blur=a.max_blur, samples=a.samples, shutter=a.shutter)
    kinds = [a.frame] if a.frame else list(FRAMES)
    planes, info = {}, {}
    for kind in kinds:
        lin, motion, z, rest = make_frame(kind, w, h, a.max_blur, a.shutter)
        planes[kind] = [torch.from_numpy(x).to(dev) for x in (lin, motion, z)] + [torch.zeros((h, w, 3), dtype=torch.float32, device=dev)]
        info[kind] = dict(at_rest=round(rest, 4), gathered=round(gathered_fraction(motion, a.max_blur, a.shutter), 4))
    torch.cuda.synchronize()
    with capi.MotionBlur(0, w, h) as mb:
        calls = {kind: (lambda p=p: mb.apply_device(stream.cuda_stream, linear_ptr=p[0].data_ptr(), motion_ptr=p[1].data_ptr(),
                                                      z_ptr=p[2].data_ptr(), out_ptr=p[3].data_ptr(), **kw)) for kind, p in planes.items()}
        ms = event_times(stream, calls, a.calls)
    res = {}
    for kind in kinds:
        n = w * h
        least = n * (12 + 12 + 12) + int(info[kind]["gathered"] * n) * 16
        t = spread(ms[kind])
        floor_us = least / a.peak_gbs / 1e3
        res[kind] = dict(call_ms=t, bytes_least=least, byte_floor_us=round(floor_us, 2), gbs_at_median=round(least / (t["median"] * 1e6), 1),
                         fraction_of_peak=round(floor_us / (t["median"] * 1e3), 4), **info[kind])
    return dict(width=w, height=h, peak_gbs=a.peak_gbs, launches_per_call=3, frames=res, **kw)


def kernel_trace(a, kind):
    """one child under rocprofv3 --kernel-trace running `kind` alone: {kernel: median us over its dispatches}"""
    child = ["--calls", a.trace_calls, "--width", a.width, "--height", a.height, "--max-blur", a.max_blur, "--samples", a.samples,
             "--shutter", a.shutter, "--frame", kind]
    with kernel_trace_db(__file__, child, prefix="mblur_trace_") as db:
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
    ap.add_argument("--max-blur", type=int, default=16)
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--shutter", type=float, default=0.5)
    ap.add_argument("--frame", default=None, choices=FRAMES, help="measure this frame alone (what the trace children do)")
    ap.add_argument("--peak-gbs", type=float, default=8685.0, help="the streaming peak the byte floor is set against (profiles/r04_peaks.json)")
    ap.add_argument("--trace-calls", type=int, default=0, help="calls of the extra children run under rocprofv3 --kernel-trace; 0: none")
    a = ap.parse_args()
    res = dict(what="tools_motion_blur_timing.py", **measure(a))
    if a.trace_calls and not a.frame:
        res["kernel_trace_command"] = "rocprofv3 --kernel-trace -d DIR -o trace -- python tools_motion_blur_timing.py --calls %d --frame FRAME" % a.trace_calls
        for kind in FRAMES:
            res["frames"][kind]["kernel_trace_us"] = kernel_trace(a, kind)
    emit(res, a.out)


if __name__ == "__main__":
    main()
