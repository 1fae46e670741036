#!/usr/bin/env python3
"""Measures what posing a skinned mesh on the device costs (rt_mi355x.h, "mesh skinning"), beside what a caller had to do before,
and writes one JSON document.
  Two scenes: the 102 k-triangle stand-in (workloads.make_balls_scene: mesh 0 is skinned, 51 202 triangles) and the Cornell box (its
  teapot is skinned).  The rig is workloads.bone_chain with 32 bones, the poses workloads.chain_pose at angles that change call by
  call.  Per scene and per mode -- STORED, SMOOTH, SMOOTH with keep_previous -- two copies of the scene, lowered, in ONE process,
  the two paths alternating call by call; medians of `--calls` after `--warmup` (min and max beside them), wall time of the call
  (it returns after the device has finished):
    (a) host      capi.mesh_skin on the host, then Scene.update_mesh_vertices with its positions: what a user does without the
                  feature; the host part alone is timed too
    (b) pose      Scene.pose_mesh: 48 bytes a bone go up, k_mesh_pose writes the positions; and that kernel's own time by the
                  library's HIP events (Scene.mesh_skin_ms), with the update's other events beside it
  One kernel, no variants.
usage: python tools_skin_timing.py [--calls 30] [--warmup 5] [--bones 32] [--out profiles/skin_timing.json]"""
import argparse
import time

from tools_timing import emit, repo_on_path, spread

MODES = {"stored": ("stored", False), "smooth": ("smooth", False), "smooth_keep_previous": ("smooth", True)}


def measure_mode(make, a, mode, keep):
    import numpy as np
    from raytracing_folder_amd import capi, workloads
    scenes = {k: make()[0] for k in ("host", "pose")}
    m = scenes["host"].export()["meshes"][0]
    v0 = m["v"]
    idx, w = workloads.bone_chain(v0, a.bones)
    origin, ray = v0.mean(0), np.array([[0, 0, 0, 0, 0, 1]], np.float32)
    for s in scenes.values():
        s.trace_rays(ray)                                          # lowered: updates from here on happen on the device
        s.set_mesh_normals(0, mode)
    scenes["pose"].set_mesh_skin(0, idx, w, a.bones)
    poses = [workloads.chain_pose(a.bones, 0.002 * (k % 11), origin, (0.0, 0.3, 1.0)) for k in range(a.warmup + a.calls)]
    wall = dict(host=[], host_skin_only=[], pose=[])
    events = dict(skin=[], upload=[], retri=[], refit=[])
    for i, bones in enumerate(poses):
        t0 = time.perf_counter()
        v = capi.mesh_skin(v0, idx, w, bones)
        t1 = time.perf_counter()
        scenes["host"].update_mesh_vertices(0, v, keep_previous=keep)
        t2 = time.perf_counter()
        scenes["pose"].pose_mesh(0, bones, keep_previous=keep)
        t3 = time.perf_counter()
        if i >= a.warmup:
            for k, dt in (("host", t2 - t0), ("host_skin_only", t1 - t0), ("pose", t3 - t2)):
                wall[k].append(dt * 1e3)
            events["skin"].append(scenes["pose"].mesh_skin_ms())
            t = scenes["pose"].mesh_update_ms()
            for k in ("upload", "retri", "refit"):
                events[k].append(t[k])
    a_, b_ = scenes["pose"].mesh_device_read(0), scenes["host"].mesh_device_read(0)
    res = dict(wall_ms={k: spread(x) for k, x in wall.items()}, pose_events_ms={k: spread(x) for k, x in events.items()},
               store_current_after_pose=scenes["pose"].mesh_skin(0)["store_current"],
               pose_equals_host=bool(all(a_[k].tobytes() == b_[k].tobytes() for k in ("tris", "nrm", "root_box"))))
    res["host_over_pose"] = round(res["wall_ms"]["host"]["median"] / res["wall_ms"]["pose"]["median"], 2)
    for s in scenes.values():
        s.close()
    return res, int(len(m["f"])), int(len(v0))


def measure_scene(make, a):
    res = {}
    for name, (mode, keep) in MODES.items():
        res[name], res["triangles"], res["vertices"] = measure_mode(make, a, mode, keep)
    # the kernel against its byte floor: 48 bytes a vertex (12 rest, 8 indices, 16 weights, 12 out) at the 8 TB/s of the part
    us = res["stored"]["pose_events_ms"]["skin"]["median"] * 1e3
    res["skin_bytes"] = 48 * res["vertices"]
    res["skin_floor_us_at_8TBs"] = round(res["skin_bytes"] / 8.0e6, 3)
    res["skin_over_floor"] = round(us / (res["skin_bytes"] / 8.0e6), 1)
    return res


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
    res = dict(what="tools_skin_timing.py", calls=a.calls, warmup=a.warmup, bones=a.bones,
               balls_102k=measure_scene(lambda: workloads.make_balls_scene(400, 300), a),
               cornell_teapot=measure_scene(lambda: workloads.load_cornell(400, 300), a))
    emit(res, a.out)


if __name__ == "__main__":
    main()
