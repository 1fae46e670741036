#!/usr/bin/env python3
"""Measures a mesh's tree built on the device against the host path it replaces, and writes one JSON document.
  Two scenes, as tools_refit_timing.py: the 102 k-triangle stand-in (mesh 0 deforms, 51 202 triangles) and the Cornell box (its
  teapot deforms).  Per scene, medians of `--calls` after `--warmup` (min and max beside them), the two paths ALTERNATING call by
  call in one process on the same vertices:
    (a) device_build  wall time of Scene.update_mesh_vertices(rebuild="device") (it returns after the device has finished, its two
                      synchronisations included) and the library's own HIP events inside it, phase by phase; launches and syncs
    (b) host_rebuild  Scene.update_mesh_vertices(rebuild=True) plus the next lowering (a one-ray trace_rays, which lowers the scene
                      and does next to nothing else): binned SAH on one host thread, then every mesh, texture and material again
    (c) cost          the SAH cost (k_bvh_cost's definition, by the host mirror) of the LBVH against the host's SAH tree
    (d) frames        the frame at 64 spp with amplitude 0, 0.1 and 0.3 of the mesh's extent under the device-built tree, the
                      refitted tree of the undeformed mesh, and the host-rebuilt tree, for the same vertices
usage: python tools_device_build_timing.py [--calls 20] [--warmup 3] [--frame-calls 5] [--out profiles/device_build_timing.json]"""
import argparse

from tools_timing import emit, repo_on_path, spread, timed

AMPLITUDES = (0.0, 0.1, 0.3)
PHASES = ("upload_ms", "sort_ms", "hierarchy_ms", "collapse_ms", "slots_ms", "cost_ms")


def measure_scene(name, make, a):
    import time

    import numpy as np
    from raytracing_folder_amd import capi, workloads
    s, cam = make()
    m = s.export()["meshes"][0]
    v0, ext = m["v"], float((m["v"].max(0) - m["v"].min(0)).max())
    p = capi.default_params(min_sample=64, max_sample=64, threshold=-1.0)
    ray = np.array([[0, 0, 0, 0, 0, 1]], np.float32)
    s.trace_rays(ray)
    n = a.warmup + a.calls
    wave = [workloads.deform_wave(v0, 0.1 * k, 0.05 * ext) for k in range(n)]
    dev, host, events, info, fell_back = [], [], {k: [] for k in PHASES}, None, 0
    for i in range(n):                                             # alternating: device build, then the host path, on the same vertices
        t0 = time.perf_counter()
        b = s.update_mesh_vertices(0, wave[i], rebuild="device")
        t1 = time.perf_counter()
        s.update_mesh_vertices(0, wave[i], rebuild=True)
        s.trace_rays(ray)
        t2 = time.perf_counter()
        if not b["on_device"]:                                     # stack_need above the limit: the call took the host path itself
            fell_back += 1
        elif i >= a.warmup:
            dev.append(1e3 * (t1 - t0)); host.append(1e3 * (t2 - t1)); info = b
            for k in PHASES:
                events[k].append(b[k])
    res = dict(triangles=int(len(m["f"])), vertices=int(len(v0)), device_build_ms=spread(dev), host_rebuild_ms=spread(host))
    res["device_build_events_ms"] = {k: spread(x) for k, x in events.items()}
    res["launches"], res["syncs"], res["levels"], res["n_nodes"], res["stack_need"] = (info[k] for k in ("launches", "syncs", "levels", "n_nodes", "stack_need"))
    res["fell_back_calls"] = fell_back
    res["host_over_device"] = round(res["host_rebuild_ms"]["median"] / res["device_build_ms"]["median"], 1)
    frames = {}
    for amp in AMPLITUDES:
        v = workloads.deform_wave(v0, 0.3, amp * ext)
        linfo, lnodes, _ = capi.device_lbvh_build(v, m["f"])
        s.update_mesh_vertices(0, v0, rebuild=True)
        s.trace_rays(ray)                                          # the host's tree of the undeformed mesh ...
        s.update_mesh_vertices(0, v)                               # ... refitted to the deformed one
        refit = timed(lambda i: s.render(cam, p), a.frame_calls, 1)
        s.update_mesh_vertices(0, v, rebuild="device")             # the same vertices under the device-built tree
        built = timed(lambda i: s.render(cam, p), a.frame_calls, 1)
        s.update_mesh_vertices(0, v, rebuild=True)                 # ... and under the host's tree built for them
        fresh = timed(lambda i: s.render(cam, p), a.frame_calls, 1)
        hn, _, hinfo = s.mesh_device_bvh(0)
        lc, hc = capi.device_bvh_cost(lnodes, linfo.root_ref)[0], capi.device_bvh_cost(hn, hinfo.root_ref)[0]
        frames[str(amp)] = dict(refit_ms=refit, device_built_ms=built, host_rebuilt_ms=fresh, lbvh_cost=lc, sah_cost=hc, cost_ratio=round(lc / hc, 4),
                                device_built_over_host=round(built["median"] / fresh["median"], 4), refit_over_host=round(refit["median"] / fresh["median"], 4))
    res["frame_64spp"] = dict(width=cam.width, height=cam.height, amplitudes=frames)
    s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frame-calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    repo_on_path()
    from raytracing_folder_amd import capi, workloads
    if capi.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing is measured (there is no CPU path)")
    res = dict(what="tools_device_build_timing.py", calls=a.calls, warmup=a.warmup, frame_calls=a.frame_calls,
               balls_102k=measure_scene("balls", lambda: workloads.make_balls_scene(400, 300), a),
               cornell_teapot=measure_scene("cornell", lambda: workloads.load_cornell(400, 300), a))
    emit(res, a.out)


if __name__ == "__main__":
    main()
