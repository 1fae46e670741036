#!/usr/bin/env python3
"""Measures what the un-interleave of a gathered multi-GPU frame costs, and writes one JSON document.
  A 1920x1080 frame in 32x8 tiles gathered from 8 ranks (device-resident, random bytes: the kernels only move them), three
  calls, interleaved in one run on one stream:
    linear_parent   rt_tiles_unpack_linear_device: k_unpack_tiles<true>, 24-byte records -> rgb8, z, count, linear
    planes_all      rt_tiles_unpack_outputs_device with all six planes: k_unpack_planes, records + five sections -> nine planes
    planes_linear   rt_tiles_unpack_outputs_device with {linear}: the same buffer and the same outputs as linear_parent
  HIP events around `--batch` back-to-back launches of one call (one launch is tens of microseconds: too short for an event
  pair of its own), `--reps` such batches per call after 10 launches of warm-up; per launch: median, min and max over the batches.
  Bytes per pixel are counted from the format (read: the record and every section; written: the planes), and the document
  gives picoseconds per byte moved beside the times -- the yardstick: planes_all must not take longer per byte than
  linear_parent, which makes the same kind of access on fewer bytes.  The outputs of planes_linear are compared with
  linear_parent's byte for byte before anything is timed.
usage: python tools_unpack_timing.py [--reps 50] [--batch 20] [--out profiles/unpack_planes_timing.json]"""
import argparse

from tools_timing import add_common_args, emit, event_times, repo_on_path, spread

ALL = ("linear", "normal", "albedo", "alpha", "object_id", "variance")
PLANE_BYTES = {"linear": 12, "normal": 12, "albedo": 12, "alpha": 4, "object_id": 4, "variance": 12}


def bytes_per_pixel(planes):
    """(read, written) by an un-interleave with `planes`: the record (24 with linear, else 8) and the sections; rgb8, z, count
    and the planes (the record's 4 zero bytes are read and not written)"""
    read = (24 if "linear" in planes else 8) + sum(PLANE_BYTES[k] for k in planes if k != "linear")
    return read, 8 + sum(PLANE_BYTES[k] for k in planes)


def measure(a):
    repo_on_path()
    import torch
    from raytracing_folder_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing is measured (there is no CPU path)")
    w, h, world, tw, th = a.width, a.height, a.world, 32, 8
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    tiles = capi.TileRange(tw, th, 0, world)
    sizes = {name: capi.tiles_packed_planes_size(w, h, tiles, planes) for name, planes in (("all", ALL), ("linear", ("linear",)))}
    per_rank = sizes["all"][1]
    gathered = {name: torch.randint(0, 256, (world * s[0],), dtype=torch.uint8, device=dev, generator=g) for name, s in sizes.items()}

    def planes():
        t = dict(rgb=torch.zeros((h, w, 3), dtype=torch.uint8, device=dev), z=torch.zeros((h, w), dtype=torch.float32, device=dev),
                 count=torch.zeros((h, w), dtype=torch.uint8, device=dev), alpha=torch.zeros((h, w), dtype=torch.float32, device=dev),
                 object_id=torch.zeros((h, w), dtype=torch.int32, device=dev))
        for k in ("linear", "normal", "albedo", "variance"):
            t[k] = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
        return t

    out_parent, out_new = planes(), planes()
    geo = (world, per_rank, w, h, tw, th)

    def new_call(which, names, out):
        return lambda: capi.tiles_unpack_outputs_device(0, stream.cuda_stream, gathered[which].data_ptr(), *geo, out["rgb"].data_ptr(),
                                                        out["z"].data_ptr(), out["count"].data_ptr(), planes=names,
                                                        **{k + "_ptr": out[k].data_ptr() for k in names})

    calls = dict(
        linear_parent=lambda: capi.tiles_unpack_device(0, stream.cuda_stream, gathered["linear"].data_ptr(), *geo, out_parent["rgb"].data_ptr(),
                                                       out_parent["z"].data_ptr(), out_parent["count"].data_ptr(),
                                                       linear_ptr=out_parent["linear"].data_ptr()),
        planes_all=new_call("all", ALL, out_new),
        planes_linear=new_call("linear", ("linear",), out_new))
    torch.cuda.synchronize()
    # the same bytes first: {linear} contributions are the 24-byte records the parent's kernel reads
    calls["linear_parent"]()
    calls["planes_linear"]()
    stream.synchronize()
    same = all(torch.equal(out_parent[k].view(torch.uint8), out_new[k].view(torch.uint8)) for k in ("rgb", "z", "count", "linear"))
    if not same:
        raise SystemExit("planes_linear and linear_parent disagree: nothing is timed")
    us = {k: [t * 1e3 / a.batch for t in v] for k, v in event_times(stream, calls, a.reps, batch=a.batch).items()}
    res = {}
    for k, names in (("linear_parent", ("linear",)), ("planes_all", ALL), ("planes_linear", ("linear",))):
        rd, wr = bytes_per_pixel(names)
        r = dict(us_per_launch=spread(us[k], 3), bytes_read_per_pixel=rd, bytes_written_per_pixel=wr)
        moved = (rd + wr) * w * h
        r["ps_per_byte"] = round(r["us_per_launch"]["median"] * 1e6 / moved, 3)
        r["gb_per_s"] = round(moved / (r["us_per_launch"]["median"] * 1e-6) / 1e9, 1)
        res[k] = r
    return dict(width=w, height=h, tile=[tw, th], world=world, tiles_per_rank=per_rank, reps=a.reps, batch=a.batch,
                all_gather_bytes_per_pixel=dict(records_linear=24, all_planes=68), outputs_identical_linear=same, calls=res,
                per_byte_all_over_parent=round(res["planes_all"]["ps_per_byte"] / res["linear_parent"]["ps_per_byte"], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=20)
    add_common_args(ap, calls=None)
    ap.add_argument("--world", type=int, default=8)
    a = ap.parse_args()
    res = dict(what="tools_unpack_timing.py", **measure(a))
    emit(res, a.out)


if __name__ == "__main__":
    main()
