#!/usr/bin/env python3
"""Measures what the motion plane of a scene with a deforming mesh costs, and writes one JSON document.  The scene is the 102 k-triangle
stand-in (workloads.make_balls_scene: mesh 0, 51 202 triangles, is the one that deforms, by workloads.deform_wave at 0.05 of its
extent) as its own camera sees it at 1920x1080; z and object_id are those of a 1 spp render and stay on the device.  The method is
tools_motion_timing.py's: HIP events on the call's stream around each call, `--calls` calls after 10 of warm-up, the kinds of call
alternating, the whole measurement `--reps` times over; and `batch`: --batch calls of one kind back to back between one event pair,
divided by their number -- the closer upper bound of a kernel's time (a pair around ONE call also times the host's way to the launch).
  k_motion              capi.motion_device on the frame (the previous camera 0.3 aside, so that the steps run, not the shortcut)
  k_motion_mesh_rigid   Scene.motion_device on the same frame with no flagged mesh: every pixel takes the rigid branch
  k_motion_mesh         Scene.motion_device after update_mesh_vertices(keep_previous=True): the pixels of mesh 0 (their share of the
                        frame is recorded) walk its tree; z and object_id are rendered again for the deformed shape
  k_motion_mesh_filled  the same with the mesh FILLING the frame: the other mesh's node emptied and the camera looking straight down
                        on the flagged mesh from 28 above its ground quad, every pixel a mesh pixel
  update                wall time of Scene.update_mesh_vertices without and with keep_previous, alternating, and the library's own
                        events around the upload (Scene.mesh_update_ms), inside which the previous positions travel
usage: python tools_motion_mesh_timing.py [--calls 100] [--reps 3] [--batch 100] [--out profiles/motion_mesh_timing.json]"""
import argparse
import statistics
import time

from tools_timing import add_common_args, emit, event_times, repo_on_path, spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=100)
    add_common_args(ap, calls=100)
    a = ap.parse_args()
    repo_on_path()
    import numpy as np
    import torch
    from raytracing_folder_amd import capi, workloads
    if capi.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing is measured (there is no CPU path)")
    w, h = a.width, a.height
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    s, cam = workloads.make_balls_scene(w, h)
    prev_cam = capi._copy_camera(cam)
    prev_cam.pos[0] += 0.3
    nodes = s.get_nodes()
    mesh_node = [i for i in range(len(nodes)) if nodes[i]["obj_type"] == capi.OBJ_MESH and nodes[i]["mesh"] == 0][0]
    m = s.export()["meshes"][0]
    v0, ext = m["v"], float((m["v"].max(0) - m["v"].min(0)).max())
    p = capi.default_params(min_sample=1, max_sample=1, threshold=-1.0)
    res = dict(what="tools_motion_mesh_timing.py", width=w, height=h, triangles=int(len(m["f"])), vertices=int(len(v0)))

    view = [cam, prev_cam]

    def planes():
        out = s.render_outputs(view[0], p, ("object_id",))
        return torch.from_numpy(out["z"]).to(dev), torch.from_numpy(out["object_id"]).to(dev), float((out["object_id"] == mesh_node).mean())

    mv = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)

    def measure(kinds, call):
        calls = {k: (lambda k=k: call(k)) for k in kinds}
        reps = [{k: spread(v) for k, v in event_times(stream, calls, a.calls, warmup=0 if r else 10).items()} for r in range(a.reps)]
        batch = {k: [t / a.batch for t in v] for k, v in event_times(stream, calls, a.reps, warmup=0, batch=a.batch).items()}
        return {k: dict(repetitions=[r[k] for r in reps], median_of_medians=round(statistics.median(r[k]["median"] for r in reps), 4),
                        batch_ms_per_call=dict(calls=a.batch, median=round(statistics.median(batch[k]), 4), min=round(min(batch[k]), 4),
                                               max=round(max(batch[k]), 4))) for k in kinds}

    # the frame at rest: k_motion against k_motion_mesh with nothing flagged
    z, ids, share = planes()
    torch.cuda.synchronize()

    def call(kind):
        kw = dict(z_ptr=z.data_ptr(), object_id_ptr=ids.data_ptr(), motion_ptr=mv.data_ptr(), sync=False)
        if kind == "k_motion":
            capi.motion_device(0, stream.cuda_stream, view[0], view[1], nodes, None, **kw)
        else:
            s.motion_device(0, stream.cuda_stream, view[0], view[1], None, **kw)
    res["mesh_pixel_share"] = round(share, 4)
    res.update(measure(("k_motion", "k_motion_mesh_rigid"), call))
    # the flag's cost on an update: without and with, alternating
    wave = [workloads.deform_wave(v0, 0.1 * k, 0.05 * ext) for k in range(8)]
    wall, upload = dict(plain=[], keep_previous=[]), dict(plain=[], keep_previous=[])
    for i in range(2 * (3 + 20)):
        kind = "keep_previous" if i & 1 else "plain"
        t0 = time.perf_counter()
        s.update_mesh_vertices(0, wave[i % 8], keep_previous=bool(i & 1))
        dt = (time.perf_counter() - t0) * 1e3
        if i >= 6:
            wall[kind].append(dt)
            upload[kind].append(s.mesh_update_ms()["upload"])
    res["update_ms"] = {k: spread(x) for k, x in wall.items()}
    res["update_upload_event_ms"] = {k: spread(x) for k, x in upload.items()}
    # the deformed frame with mesh 0 flagged
    s.update_mesh_vertices(0, wave[2])
    s.update_mesh_vertices(0, wave[3], keep_previous=True)
    z, ids, share = planes()
    torch.cuda.synchronize()
    res["mesh_pixel_share_deformed"] = round(share, 4)
    res.update(measure(("k_motion_mesh",), call))
    found = mv[..., 2][ids == mesh_node] > 0
    res["mesh_pixels_with_a_previous_position"] = round(float(found.float().mean().item()), 4)
    # the flagged mesh filling the frame
    only = nodes.copy()
    for i in range(len(only)):
        if only[i]["obj_type"] == capi.OBJ_MESH and only[i]["mesh"] != 0:
            only[i]["obj_type"] = capi.OBJ_NONE
    s.set_nodes(only)
    for c, x in zip(view, (0.0, 0.3)):
        c.pos[:], c.dir[:], c.up[:] = (x, -4.0, 28.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0)
    z, ids, share = planes()
    torch.cuda.synchronize()
    res["mesh_pixel_share_filled"] = round(share, 4)
    res.update(measure(("k_motion_mesh_filled",), call))
    res["filled_mesh_pixels_with_a_previous_position"] = round(float((mv[..., 2][ids == mesh_node] > 0).float().mean().item()), 4)
    s.close()
    emit(res, a.out)


if __name__ == "__main__":
    main()
