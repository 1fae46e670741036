#!/usr/bin/env python3
"""Measures what posing a mesh with morph targets on the device costs (rt_mi355x.h, "morph targets"), beside what a caller had to
do before, and writes one JSON document.
  Two scenes: the 102 k-triangle stand-in (workloads.make_balls_scene: mesh 0, 51 202 triangles) and the Cornell box (its teapot).
  The set is workloads.morph_targets with 256 targets; 4, 32 or 256 of them are active (evenly spread over the 256), with weights
  that change call by call; each with and without a skin of workloads.bone_chain with 32 bones posed by workloads.chain_pose.  The
  meshes are in SMOOTH mode.  Per case two copies of the scene, lowered, in ONE process, the two paths alternating call by call;
  medians of `--calls` after `--warmup` (min and max beside them), wall time of the call (it returns after the device has
  finished):
    (a) host      capi.mesh_morph (and capi.mesh_skin) on the host, then Scene.update_mesh_vertices with the positions: what a user
                  does without the feature; the host part alone is timed too
    (b) pose      Scene.pose_mesh(morph_weights=...): 8 bytes an active target and 48 a bone go up, k_mesh_pose writes the
                  positions; and that kernel's own time by the library's HIP events (Scene.mesh_morph_ms), with the update's other
                  events beside it
  The kernel against its bytes: 12 (n_active + 2) a vertex, + 24 with a skin, at a rate taken from profiles/r04_peaks.json.  That
  file holds no streaming HBM figure; the rate used is gather_shape_5_waves_per_simd.random_over_34MB.chip_GBps (8685 GB/s), a
  random gather over 34 MB -- its one figure for loads that miss the 4 MB L2, served largely by the 256 MB last-level cache and so
  ABOVE what HBM itself streams (8 TB/s nominal).  The floor it gives is therefore a low one and the ratios to it are upper
  bounds of the ratio to a true HBM floor by under a tenth; the document records the rate and its name.
  One kernel, no variants.
usage: python tools_morph_timing.py [--calls 30] [--warmup 5] [--bones 32] [--out profiles/morph_timing.json]"""
import argparse
import json
import os
import time

from tools_timing import emit, repo_on_path, spread

N_TARGETS = 256
ACTIVE = (4, 32, 256)


def measure_case(make, a, n_active, with_skin, deltas_of):
    import numpy as np
    from raytracing_folder_amd import capi, workloads
    scenes = {k: make()[0] for k in ("host", "pose")}
    m = scenes["host"].export()["meshes"][0]
    v0 = m["v"]
    deltas = deltas_of(v0)
    idx, sw = workloads.bone_chain(v0, a.bones)
    origin, ray = v0.mean(0), np.array([[0, 0, 0, 0, 0, 1]], np.float32)
    for s in scenes.values():
        s.trace_rays(ray)                                          # lowered: updates from here on happen on the device
        s.set_mesh_normals(0, "smooth")
    scenes["pose"].set_mesh_morphs(0, deltas)
    if with_skin:
        scenes["pose"].set_mesh_skin(0, idx, sw, a.bones)
    on = np.arange(n_active) * (N_TARGETS // n_active)
    sign = np.where(np.arange(n_active) % 2 == 0, 1.0, -1.0)
    wall = dict(host=[], host_math_only=[], pose=[])
    events = dict(morph=[], upload=[], retri=[], refit=[])
    for i in range(a.warmup + a.calls):
        w = np.zeros(N_TARGETS, np.float32)
        w[on] = sign * (0.05 + 0.01 * (i % 11)) * (4.0 / n_active) ** 0.5
        bones = workloads.chain_pose(a.bones, 0.002 * (i % 11), origin, (0.0, 0.3, 1.0)) if with_skin else None
        t0 = time.perf_counter()
        v = capi.mesh_morph(v0, deltas, w)
        if with_skin:
            v = capi.mesh_skin(v, idx, sw, bones)
        t1 = time.perf_counter()
        scenes["host"].update_mesh_vertices(0, v)
        t2 = time.perf_counter()
        scenes["pose"].pose_mesh(0, bones, morph_weights=w)
        t3 = time.perf_counter()
        if i >= a.warmup:
            for k, dt in (("host", t2 - t0), ("host_math_only", t1 - t0), ("pose", t3 - t2)):
                wall[k].append(dt * 1e3)
            events["morph"].append(scenes["pose"].mesh_morph_ms())
            t = scenes["pose"].mesh_update_ms()
            for k in ("upload", "retri", "refit"):
                events[k].append(t[k])
    a_, b_ = scenes["pose"].mesh_device_read(0), scenes["host"].mesh_device_read(0)
    res = dict(n_active=n_active, skin=with_skin, vertices=int(len(v0)), triangles=int(len(m["f"])),
               wall_ms={k: spread(x) for k, x in wall.items()}, pose_events_ms={k: spread(x) for k, x in events.items()},
               store_current_after_pose=scenes["pose"].mesh_morphs(0)["store_current"],
               pose_equals_host=bool(all(a_[k].tobytes() == b_[k].tobytes() for k in ("tris", "nrm", "root_box"))))
    res["host_over_pose"] = round(res["wall_ms"]["host"]["median"] / res["wall_ms"]["pose"]["median"], 2)
    res["morph_bytes"] = (12 * (n_active + 2) + (24 if with_skin else 0)) * res["vertices"]
    floor_us = res["morph_bytes"] / (a.gbps * 1e3)
    res["morph_floor_us"] = round(floor_us, 3)
    res["morph_over_floor"] = round(res["pose_events_ms"]["morph"]["median"] * 1e3 / floor_us, 1)
    for s in scenes.values():
        s.close()
    return res


def measure_scene(make, a):
    from raytracing_folder_amd import workloads
    made = {}

    def deltas_of(v0):                                             # one set a scene, shared by its cases
        if "d" not in made:
            made["d"] = workloads.morph_targets(v0, N_TARGETS)
        return made["d"]
    return [measure_case(make, a, n, skin, deltas_of) for n in ACTIVE for skin in (False, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bones", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    repo_on_path()
    from raytracing_folder_amd import capi, workloads
    if capi.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing is measured (there is no CPU path)")
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r04_peaks.json")) as f:
        a.gbps = float(json.load(f)["gather_shape_5_waves_per_simd"]["random_over_34MB"]["chip_GBps"])
    res = dict(what="tools_morph_timing.py", calls=a.calls, warmup=a.warmup, bones=a.bones, targets_bound=N_TARGETS, rate_GBps=a.gbps,
               rate_is="profiles/r04_peaks.json gather_shape_5_waves_per_simd.random_over_34MB.chip_GBps: a random gather past L2, not an HBM stream",
               balls_102k=measure_scene(lambda: workloads.make_balls_scene(400, 300), a),
               cornell_teapot=measure_scene(lambda: workloads.load_cornell(400, 300), a))
    emit(res, a.out)


if __name__ == "__main__":
    main()
