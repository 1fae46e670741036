#!/usr/bin/env python3
"""Measures what recomputing a deforming mesh's smooth normals on the device costs (rt_mi355x.h, "smooth normals"), beside the
update without it and beside what a caller had to do before, and writes one JSON document.
  Two scenes: the 102 k-triangle stand-in (workloads.make_balls_scene: mesh 0 deforms, 51 202 triangles) and the Cornell box (its
  teapot deforms, fn != f).  The deformation is workloads.deform_wave.  Per scene three copies of it, lowered, in ONE process, the
  three paths alternating call by call; medians of `--calls` after `--warmup` (min and max beside them), wall time of the call
  (an update returns after the device has finished):
    (a) stored    Scene.update_mesh_vertices without normals in STORED mode: the call as it always was, stale normals
    (b) smooth    the same call in SMOOTH mode: k_mesh_normals runs between the upload and k_mesh_retri; and that kernel's own time
                  by the library's HIP events (Scene.mesh_normals_ms), with the update's other events beside it
    (c) host      correct shading without the feature: capi.mesh_smooth_normals on the host, then the update with that vn;
                  the host part alone is timed too
  The kernel recomputes a face's normal per corner; the variant that stages one normal per face first was not built.
usage: python tools_normals_timing.py [--calls 30] [--warmup 5] [--out profiles/normals_timing.json]"""
import argparse
import time

from tools_timing import emit, repo_on_path, spread


def measure_scene(make, a):
    import numpy as np
    from raytracing_folder_amd import capi, workloads
    scenes = {k: make()[0] for k in ("stored", "smooth", "host")}
    m = scenes["stored"].export()["meshes"][0]
    v0, ext = m["v"], float((m["v"].max(0) - m["v"].min(0)).max())
    ray = np.array([[0, 0, 0, 0, 0, 1]], np.float32)
    for s in scenes.values():
        s.trace_rays(ray)                                          # lowered: updates from here on happen on the device
    scenes["smooth"].set_mesh_normals(0, "smooth")
    wave = [workloads.deform_wave(v0, 0.1 * k, 0.05 * ext) for k in range(a.warmup + a.calls)]
    wall = dict(stored=[], smooth=[], host=[], host_normals_only=[])
    events = dict(normals=[], upload=[], retri=[], refit=[])
    for i, v in enumerate(wave):
        keep = i >= a.warmup
        t0 = time.perf_counter()
        scenes["stored"].update_mesh_vertices(0, v)
        t1 = time.perf_counter()
        scenes["smooth"].update_mesh_vertices(0, v)
        t2 = time.perf_counter()
        vn = capi.mesh_smooth_normals(v, m["f"], m["fn"], m["vn"])
        t3 = time.perf_counter()
        scenes["host"].update_mesh_vertices(0, v, vn)
        t4 = time.perf_counter()
        if keep:
            for k, dt in (("stored", t1 - t0), ("smooth", t2 - t1), ("host", t4 - t2), ("host_normals_only", t3 - t2)):
                wall[k].append(dt * 1e3)
            events["normals"].append(scenes["smooth"].mesh_normals_ms())
            t = scenes["smooth"].mesh_update_ms()
            for k in ("upload", "retri", "refit"):
                events[k].append(t[k])
    # the three devices hold the same normals: (b) computed what (c) was given
    a_, b_ = scenes["smooth"].mesh_device_read(0), scenes["host"].mesh_device_read(0)
    res = dict(triangles=int(len(m["f"])), vertices=int(len(v0)), normals=int(len(m["vn"])),
               wall_ms={k: spread(x) for k, x in wall.items()}, smooth_events_ms={k: spread(x) for k, x in events.items()},
               smooth_equals_host=bool(a_["nrm"].tobytes() == b_["nrm"].tobytes()))
    res["smooth_over_stored"] = round(res["wall_ms"]["smooth"]["median"] / res["wall_ms"]["stored"]["median"], 3)
    res["host_over_smooth"] = round(res["wall_ms"]["host"]["median"] / res["wall_ms"]["smooth"]["median"], 2)
    for s in scenes.values():
        s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    repo_on_path()
    from raytracing_folder_amd import capi, workloads
    if capi.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing is measured (there is no CPU path)")
    res = dict(what="tools_normals_timing.py", calls=a.calls, warmup=a.warmup, variant="recompute per corner (staged variant not built)",
               balls_102k=measure_scene(lambda: workloads.make_balls_scene(400, 300), a),
               cornell_teapot=measure_scene(lambda: workloads.load_cornell(400, 300), a))
    emit(res, a.out)


if __name__ == "__main__":
    main()
