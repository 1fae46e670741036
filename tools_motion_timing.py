#!/usr/bin/env python3
"""Measures what the motion plane costs, and writes one JSON document.  Everything on device-resident 1920x1080 planes, HIP events
on the call's stream around each call, `--calls` calls after 10 of warm-up, the three kinds of call alternating; the whole
measurement `--reps` times over, so that the spread from repetition to repetition can be set beside the differences:
  motion:           one rt_motion_device call: a wall 10 away in three objects, one of them moved by 0.3 between the frames, the
                    camera alternating between two positions 0.3 apart (the node table is the same from call to call, so no
                    call uploads it).  20 bytes a pixel: z and object_id in, three floats out.
  temporal_motion:  one rt_temporal_motion_device call with that plane, history holding a frame (no variance plane)
  temporal:         one rt_temporal_device call on the same planes: the camera-only path, as tools_temporal_timing.py measures it
                    (without_variance) -- the figure to hold against profiles/temporal_timing.json
An event pair around ONE call on an idle stream also times the host's way to the launch behind the first event (ctypes, the
node table, the launch itself): for the short k_motion that share counts, so these figures are upper bounds of the kernels'
times.  `batch` therefore also times --batch calls of one kind back to back between one event pair, divided by their number:
the launches overlap the kernels in front of them, and what is left is the larger of the kernel's time and the host's time per
call -- again an upper bound of the kernel's, and the closer one.
usage: python tools_motion_timing.py [--calls 200] [--reps 5] [--batch 200] [--out profiles/motion_timing.json]"""
import argparse
import statistics

from tools_timing import add_common_args, emit, event_times, repo_on_path, spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=200)
    add_common_args(ap, calls=200)
    a = ap.parse_args()
    repo_on_path()
    import numpy as np
    import torch
    from raytracing_folder_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing is measured (there is no CPU path)")
    w, h = a.width, a.height
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    res = dict(what="tools_motion_timing.py", width=w, height=h)

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
    ids = (1 + X * 3 // w).astype(np.int32)            # nodes 1, 2, 3 under the root
    normal = np.zeros((h, w, 3), np.float32)
    normal[..., 2] = 1
    albedo = np.float32([[0.8, 0.5, 0.3], [0.2, 0.6, 0.9], [0.7, 0.7, 0.7]])[ids - 1]
    clean = albedo * (0.6 + 0.3 * np.sin(X / 50.0) * np.cos(Y / 70.0))[..., None]
    lin = (clean * (1 + 0.3 * rng.normal(0, 1, (h, w, 3)))).astype(np.float32)
    nodes = np.zeros(4, capi.NODE)
    eye = np.eye(3, dtype=np.float32).reshape(9)
    for i in range(4):
        nodes[i]["tm"], nodes[i]["itm"], nodes[i]["parent"] = eye, eye, -1 if i == 0 else 0
    prev = nodes.copy()
    nodes[2]["pos"] = (0.3, 0.0, 0.0)
    t = {k: torch.from_numpy(v).to(dev) for k, v in dict(linear=lin, normal=normal, albedo=albedo, z=z, object_id=ids).items()}
    out, hist, mv = (torch.zeros((h, w, 3), dtype=torch.float32, device=dev), torch.zeros((h, w), dtype=torch.float32, device=dev),
                     torch.zeros((h, w, 3), dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    histories = dict(temporal=capi.History(0, w, h), temporal_motion=capi.History(0, w, h))
    count = dict(motion=0, temporal=0, temporal_motion=0)

    def call(kind):
        count[kind] += 1
        cam, other = cams[count[kind] & 1], cams[1 - (count[kind] & 1)]
        if kind == "motion":
            capi.motion_device(0, stream.cuda_stream, cam, other, nodes, prev, z_ptr=t["z"].data_ptr(), object_id_ptr=t["object_id"].data_ptr(),
                               motion_ptr=mv.data_ptr(), sync=False)
            return
        histories[kind].accumulate_device(stream.cuda_stream, cam, linear_ptr=t["linear"].data_ptr(), normal_ptr=t["normal"].data_ptr(),
                                          albedo_ptr=t["albedo"].data_ptr(), z_ptr=t["z"].data_ptr(), object_id_ptr=t["object_id"].data_ptr(),
                                          out_ptr=out.data_ptr(), history_ptr=hist.data_ptr(), sync=False,
                                          motion_ptr=mv.data_ptr() if kind == "temporal_motion" else None)

    kinds = ("motion", "temporal_motion", "temporal")
    calls = {k: (lambda k=k: call(k)) for k in kinds}
    reps = [{k: spread(v) for k, v in event_times(stream, calls, a.calls, warmup=0 if r else 10).items()} for r in range(a.reps)]
    batch = {k: [t / a.batch for t in v] for k, v in event_times(stream, calls, a.reps, warmup=0, batch=a.batch).items()}
    res["repetitions"] = reps
    res["median_ms"] = {k: dict(median_of_medians=round(statistics.median(r[k]["median"] for r in reps), 4),
                                min_of_medians=round(min(r[k]["median"] for r in reps), 4),
                                max_of_medians=round(max(r[k]["median"] for r in reps), 4)) for k in kinds}
    res["batch_ms_per_call"] = {k: dict(calls=a.batch, median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
                                for k, v in batch.items()}
    res["mean_history"] = float(hist.mean().item())
    # k_motion per pixel: z 4, id 4 in, motion 12 out
    res["motion_bytes_per_pixel"] = 20
    res["motion_gb_per_s"] = dict(single_call=round(20 * w * h / (res["median_ms"]["motion"]["median_of_medians"] * 1e-3) / 1e9, 1),
                                  batch=round(20 * w * h / (res["batch_ms_per_call"]["motion"]["median"] * 1e-3) / 1e9, 1))
    for k in histories.values():
        k.close()
    emit(res, a.out)


if __name__ == "__main__":
    main()
