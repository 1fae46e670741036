#!/usr/bin/env python3
"""Measures what history rectification costs on top of the plain temporal accumulation, and what it buys, and writes one JSON
document.  The method is tools_temporal_timing.py's:
  accumulate: one rt_temporal_clip_device call on device-resident 1920x1080 planes with a history that holds a frame, the camera
              alternating between two positions 0.3 apart (every call reprojects and gathers), for radius 1, 2 and 3, with the
              cameras' reprojection and with a motion plane, and -- in the same run, the variants alternating -- the plain
              rt_temporal_device / rt_temporal_motion_device call beside them; no variance plane; HIP events on the call's stream
              around each call, `--calls` calls after 10 of warm-up; median, min and max.
              Bytes: what a pixel moves.  The plain kernel: tools_temporal_timing.py's count (+ 12 for a motion plane).  The
              rectified one adds the mask (4) and the staging of the halo: rgb, albedo and id (28 bytes) of (32+2r)(8+2r) pixels
              for every 256 -- counted in full, although the tile's own 256 pixels are read a second time by their lanes and the
              halo's by the neighbouring workgroups, so most of it is served by the caches.
  quality:    tests/test_temporal_clip.py's moved_light_rmse(): cornell_gi.xml at 96x72, the point light moved after four of
              six 4 spp frames, RMSE to 64 spp under the new light of the plain and the rectified accumulation; and eight static
              frames, rectified, against one frame.
  resources:  --asm-remarks FILE: the compiler's kernel-resource-usage remarks of rt_temporal.hip (the stderr of `make asm` in
              raytracing_folder_amd/csrc); VGPRs, SGPRs, scratch, LDS bytes and waves per SIMD of the k_temporal* kernels are copied
              into the document.
usage: python tools_temporal_clip_timing.py [--calls 200] [--no-quality] [--asm-remarks FILE] [--out profiles/temporal_clip_timing.json]"""
import argparse

from tools_timing import add_common_args, emit, event_times, repo_on_path, spread


def kernel_resources(path, only="k_temporal"):
    """{kernel: {vgprs, sgprs, scratch, lds_bytes, waves_per_simd}} from -Rpass-analysis=kernel-resource-usage remarks, for the
    kernels whose mangled name holds `only`"""
    import re
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch", "LDS Size [bytes/block]": "lds_bytes",
            "Occupancy [waves/SIMD]": "waves_per_simd"}
    res, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), {})
        elif cur is not None and m.group(1) in keys:
            cur[keys[m.group(1)]] = int(m.group(2))
    return {k: v for k, v in res.items() if only in k}


def main():
    ap = argparse.ArgumentParser()
    add_common_args(ap)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--asm-remarks", default=None)
    a = ap.parse_args()
    repo_on_path()
    import numpy as np
    import torch
    from raytracing_folder_amd import capi
    from tests import test_temporal_clip as tc
    if capi.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing is measured (there is no CPU path)")
    w, h = a.width, a.height
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    res = dict(what="tools_temporal_clip_timing.py on one MI355X: one rt_temporal_clip_device call on device-resident planes (history holding "
                    "a frame, camera alternating between two positions, no variance plane), radius 1, 2, 3 with the cameras' reprojection and "
                    f"with a motion plane, the plain calls beside them in the same run, {a.calls} calls each, the variants alternating, HIP "
                    "events on the call's stream; quality: cornell_gi.xml 96x72, 4 spp frames against 64 spp of another seed, linear RMSE "
                    "over hit pixels (tests/test_temporal_clip.py: moved_light_rmse); kernel_resources: the compiler's report",
               width=w, height=h)

    # tools_temporal_timing.py's frame: a wall 10 away seen from two camera positions, noise 0.3
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
    ids = (X * 3 // w).astype(np.int32)
    normal = np.zeros((h, w, 3), np.float32)
    normal[..., 2] = 1
    albedo = np.float32([[0.8, 0.5, 0.3], [0.2, 0.6, 0.9], [0.7, 0.7, 0.7]])[ids]
    clean = albedo * (0.6 + 0.3 * np.sin(X / 50.0) * np.cos(Y / 70.0))[..., None]
    lin = (clean * (1 + 0.3 * rng.normal(0, 1, (h, w, 3)))).astype(np.float32)
    pl = dict(linear=lin, normal=normal, albedo=albedo, z=z, object_id=np.zeros((h, w), np.int32))
    t = {k: torch.from_numpy(v).to(dev) for k, v in pl.items()}
    # the motion plane of each camera, seen from the other one
    mv = [torch.from_numpy(tc.motion_plane(cams[i], cams[1 - i], pl)).to(dev) for i in (0, 1)]
    mk = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
    out, hist, mask = mk(h, w, 3), mk(h, w), mk(h, w)
    torch.cuda.synchronize()
    variants = [(r, m) for m in (False, True) for r in (0, 1, 2, 3)]            # radius 0: the plain kernel
    histories = {v: capi.History(0, w, h) for v in variants}
    count = {v: 0 for v in variants}

    def call(v):
        radius, motion = v
        count[v] += 1
        i = count[v] & 1
        extra = dict(clip={"radius": radius}, clipped_ptr=mask.data_ptr()) if radius else {}
        if motion:
            extra["motion_ptr"] = mv[i].data_ptr()
        histories[v].accumulate_device(stream.cuda_stream, cams[i], linear_ptr=t["linear"].data_ptr(), normal_ptr=t["normal"].data_ptr(),
                                       albedo_ptr=t["albedo"].data_ptr(), z_ptr=t["z"].data_ptr(), object_id_ptr=t["object_id"].data_ptr(),
                                       out_ptr=out.data_ptr(), history_ptr=hist.data_ptr(), sync=False, **extra)

    ms = event_times(stream, {v: (lambda v=v: call(v)) for v in variants}, a.calls)
    clipped_share = {}
    with torch.cuda.stream(stream):
        for v in variants:
            if v[0]:
                call(v)
                stream.synchronize()
                clipped_share[v] = float((mask == 2).float().mean().item())
    name = lambda v: ("plain" if v[0] == 0 else f"radius_{v[0]}") + ("_motion" if v[1] else "")
    res["accumulate_ms"] = {name(v): spread(ms[v]) for v in variants}
    res["clipped_share"] = {name(v): round(s, 4) for v, s in clipped_share.items()}
    plain = 12 * 3 + 8 + 16 + 48 + 4 * 48
    halo = lambda r: round(28 * (32 + 2 * r) * (8 + 2 * r) / 256.0, 1)
    res["bytes_per_pixel"] = {name(v): (plain + (12 if v[1] else 0) + ((4 + halo(v[0])) if v[0] else 0)) for v in variants}
    res["lds_bytes_per_workgroup"] = {f"radius_{r}": (32 + 2 * r) * (8 + 2 * r) * 16 for r in (1, 2, 3)}
    res["lds_bytes_allocated"] = 8512
    for k in histories.values():
        k.close()
    if a.asm_remarks:
        res["kernel_resources"] = kernel_resources(a.asm_remarks)
    if not a.no_quality:
        q = tc.moved_light_rmse()
        res["quality_cornell_gi_96x72"] = {k: {n: round(x, 6) for n, x in v.items()} for k, v in q.items()}
    emit(res, a.out)


if __name__ == "__main__":
    main()
