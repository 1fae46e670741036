#!/usr/bin/env python3
"""Measures what an in-place mesh vertex update costs beside the full path it replaces, and writes one JSON document.
  Two scenes: the 102 k-triangle stand-in (workloads.make_balls_scene: two meshes of 64 spheres, mesh 0 is the one that deforms,
  51 202 triangles) and the Cornell box (its teapot deforms).  The deformation is workloads.deform_wave.  Per scene, medians of
  `--calls` after `--warmup` (min and max beside them):
    (a) update    wall time of Scene.update_mesh_vertices (it returns after the device has finished), and the library's own HIP
                  events inside it (Scene.mesh_update_ms): the vertex upload, k_mesh_retri, the refit launches, and their number
    (b) rebuild   the way without it, in the same process: capi.bvh_build + Scene.set_mesh + the first lowering (a one-ray
                  trace_rays, which lowers the scene and does next to nothing else)
    (c) frames    the frame at 64 spp after a refit with amplitude 0, 0.05 and 0.3 of the mesh's extent, against the frame of a
                  fresh scene given the same vertices: what the refitted tree's looser topology costs the tracer
usage: python tools_refit_timing.py [--calls 20] [--warmup 3] [--out profiles/refit_timing.json]"""
import argparse

from tools_timing import emit, repo_on_path, spread, timed

AMPLITUDES = (0.0, 0.05, 0.3)


def measure_scene(name, make, a):
    import numpy as np
    from raytracing_folder_amd import capi, workloads
    s, cam = make()
    m = s.export()["meshes"][0]
    v0, ext = m["v"], float((m["v"].max(0) - m["v"].min(0)).max())
    p = capi.default_params(min_sample=64, max_sample=64, threshold=-1.0)
    ray = np.array([[0, 0, 0, 0, 0, 1]], np.float32)
    s.trace_rays(ray)                                              # lowered: updates from here on happen on the device
    wave = [workloads.deform_wave(v0, 0.1 * k, 0.05 * ext) for k in range(a.warmup + a.calls)]
    events = dict(upload=[], retri=[], refit=[])
    launches = []

    def update(i):
        s.update_mesh_vertices(0, wave[i])
        if i >= a.warmup:
            t = s.mesh_update_ms()
            for k in events:
                events[k].append(t[k])
            launches.append(t["level_launches"])
    res = dict(triangles=int(len(m["f"])), vertices=int(len(v0)), update_ms=timed(update, a.calls, a.warmup))
    res["update_events_ms"] = {k: spread(x) for k, x in events.items()}
    res["level_launches"] = launches[0]

    def rebuild(i):
        s.set_mesh(0, wave[i], m["f"], m["vn"], m["fn"], *capi.bvh_build(wave[i], m["f"]), m["vt"], m["ft"])
        s.trace_rays(ray)
    res["rebuild_ms"] = timed(rebuild, a.calls, a.warmup)
    res["rebuild_over_update"] = round(res["rebuild_ms"]["median"] / res["update_ms"]["median"], 1)
    frames = {}
    for amp in AMPLITUDES:
        v = workloads.deform_wave(v0, 0.3, amp * ext)
        s.set_mesh(0, v0, m["f"], m["vn"], m["fn"], *capi.bvh_build(v0, m["f"]), m["vt"], m["ft"])
        s.trace_rays(ray)                                          # the tree of the undeformed mesh ...
        s.update_mesh_vertices(0, v)                               # ... refitted to the deformed one
        refit = timed(lambda i: s.render(cam, p), a.calls, a.warmup)
        s.update_mesh_vertices(0, v, rebuild=True)                 # the same vertices under a tree built for them
        fresh = timed(lambda i: s.render(cam, p), a.calls, a.warmup)
        frames[str(amp)] = dict(refit_ms=refit, fresh_ms=fresh, refit_over_fresh=round(refit["median"] / fresh["median"], 4))
    res["frame_64spp"] = dict(width=cam.width, height=cam.height, amplitudes=frames)
    s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    repo_on_path()
    from raytracing_folder_amd import capi, workloads
    if capi.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing is measured (there is no CPU path)")
    res = dict(what="tools_refit_timing.py", calls=a.calls, warmup=a.warmup,
               balls_102k=measure_scene("balls", lambda: workloads.make_balls_scene(400, 300), a),
               cornell_teapot=measure_scene("cornell", lambda: workloads.load_cornell(400, 300), a))
    emit(res, a.out)


if __name__ == "__main__":
    main()
