#!/usr/bin/env python3
"""Measures the mesh tree quality measure (k_bvh_cost, Scene.mesh_quality, Scene.update_mesh_vertices(max_ratio=)) and writes one
JSON document.  The scenes, the deformation and the way of timing are tools_refit_timing.py's: the 102 k-triangle stand-in (mesh 0,
51 202 triangles, deforms) and the Cornell box (its teapot deforms); medians of `--calls` after `--warmup`, min and max beside them.
Per scene:
    (a) measure   k_bvh_cost and the copies behind it by the library's HIP events (rt_mesh_quality.measure_ms), per call of an
                  update with max_ratio, beside the upload / retri / refit events of the SAME calls, and the bytes the kernel must
                  read (128 a node record); the wall time of Scene.mesh_quality() on its own
    (b) update    wall time of Scene.update_mesh_vertices without max_ratio and with it (max_ratio so large that nothing is built
                  again), each its own median over its own calls
    (c) table     per amplitude 0, 0.05, 0.1, 0.2 and 0.3 of the extent: the SAH ratio of the refitted tree, and the frame at
                  64 spp after the refit over the frame after a rebuild for the same vertices (tools_refit_timing.py's (c))
`--fold` only labels the document: which build of the library ran (RT_MI355X_LIB selects `make cost_fold_device`'s, whose block
sums are folded by k_bvh_cost_fold on the device instead of by the host); with --skip-table such a run measures (a) and (b) only.
usage: python tools_refit_quality.py [--calls 20] [--warmup 3] [--fold host] [--skip-table] [--out profiles/refit_quality.json]"""
import argparse

from tools_timing import emit, repo_on_path, spread, timed

AMPLITUDES = (0.0, 0.05, 0.1, 0.2, 0.3)


def measure_scene(make, a):
    import numpy as np
    from raytracing_folder_amd import capi, workloads
    s, cam = make()
    m = s.export()["meshes"][0]
    v0, ext = m["v"], float((m["v"].max(0) - m["v"].min(0)).max())
    p = capi.default_params(min_sample=64, max_sample=64, threshold=-1.0)
    ray = np.array([[0, 0, 0, 0, 0, 1]], np.float32)
    s.trace_rays(ray)                                              # lowered: updates from here on happen on the device
    n_nodes = int(s.mesh_device_bvh(0)[2].n_nodes)
    wave = [workloads.deform_wave(v0, 0.1 * k, 0.05 * ext) for k in range(a.warmup + a.calls)]
    res = dict(triangles=int(len(m["f"])), vertices=int(len(v0)), node_records=n_nodes, bytes_read=128 * n_nodes,
               blocks=(4 * n_nodes + 255) // 256, bytes_written=8 * ((4 * n_nodes + 255) // 256))
    res["update_plain_ms"] = timed(lambda i: s.update_mesh_vertices(0, wave[i]), a.calls, a.warmup)
    events = dict(upload=[], retri=[], refit=[], measure=[])

    def auto(i):
        q = s.update_mesh_vertices(0, wave[i], max_ratio=1e30)
        if i >= a.warmup:
            t = s.mesh_update_ms()
            for k in ("upload", "retri", "refit"):
                events[k].append(t[k])
            events["measure"].append(q["measure_ms"])
    res["update_max_ratio_ms"] = timed(auto, a.calls, a.warmup)
    res["events_ms"] = {k: spread(x) for k, x in events.items()}
    res["gb_per_s"] = round(res["bytes_read"] / (res["events_ms"]["measure"]["median"] * 1e-3) / 1e9, 2)
    query = []
    res["mesh_quality_call_ms"] = timed(lambda i: query.append(s.mesh_quality(0)["measure_ms"]), a.calls, a.warmup)
    res["mesh_quality_events_ms"] = spread(query[a.warmup:])
    res["update_plain_again_ms"] = timed(lambda i: s.update_mesh_vertices(0, wave[i]), a.calls, a.warmup)
    if not a.skip_table:
        table = {}
        for amp in AMPLITUDES:
            v = workloads.deform_wave(v0, 0.3, amp * ext)
            s.set_mesh(0, v0, m["f"], m["vn"], m["fn"], *capi.bvh_build(v0, m["f"]), m["vt"], m["ft"])
            s.trace_rays(ray)                                      # the tree of the undeformed mesh ...
            q = s.update_mesh_vertices(0, v, max_ratio=1e30)       # ... refitted to the deformed one, and measured
            refit = timed(lambda i: s.render(cam, p), a.calls, a.warmup)
            s.update_mesh_vertices(0, v, rebuild=True)             # the same vertices under a tree built for them
            fresh = timed(lambda i: s.render(cam, p), a.calls, a.warmup)
            table[str(amp)] = dict(sah_ratio=round(q["ratio"], 6), cost=round(q["cost"], 6), built_cost=round(q["built_cost"], 6),
                                   fresh_cost=round(s.mesh_quality(0)["cost"], 6), refit_ms=refit, fresh_ms=fresh,
                                   refit_over_fresh=round(refit["median"] / fresh["median"], 4))
        res["frame_64spp"] = dict(width=cam.width, height=cam.height, amplitudes=table)
        ratios = [table[str(amp)]["sah_ratio"] for amp in AMPLITUDES]
        frames = [table[str(amp)]["refit_over_fresh"] for amp in AMPLITUDES]
        order = sorted(range(len(AMPLITUDES)), key=lambda k: ratios[k])
        res["sah_ratio_orders_frame_ratio"] = all(frames[order[k]] <= frames[order[k + 1]] for k in range(len(order) - 1))
    s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fold", default="host", help="label only: where the library that ran folds the block sums (host | device)")
    ap.add_argument("--skip-table", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    repo_on_path()
    from raytracing_folder_amd import capi, workloads
    if capi.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing is measured (there is no CPU path)")
    res = dict(what="tools_refit_quality.py", calls=a.calls, warmup=a.warmup, fold=a.fold,
               balls_102k=measure_scene(lambda: workloads.make_balls_scene(400, 300), a),
               cornell_teapot=measure_scene(lambda: workloads.load_cornell(400, 300), a))
    emit(res, a.out)


if __name__ == "__main__":
    main()
