"""Multi-GPU sharding of a frame: interleaved tiles + one all-gather of the finished tiles.

The reference parallelises over pixels with one shared atomic counter (FIN/main.cpp:65-85; FIN =
/root/reference/RayTracingFinal/RayTracingFinal).  Here the image is cut into tile_w x tile_h
tiles numbered row-major; rank r of R renders tiles r, r+R, r+2R, ... (interleaved, so that the
expensive glass/mirror pixels spread over all ranks), every rank holds the whole scene and photon
map, and the only exchange is ONE all_gather of each rank's finished tiles -- 8 bytes per pixel
(RGB8 + float z + sample-count byte) -- over RCCL/xGMI (backend "nccl" on ROCm) or gloo on CPU.
torch is plumbing here: device buffers, the stream handle and torch.distributed.

A frame that is to be denoised, accumulated or followed by motion vectors also needs its linear, first-hit and variance
planes on every rank: they travel in the same all-gather as sections behind the records (the "packed planes" format of
include/rt_mi355x.h; pack_own_planes / unpack_gathered_planes are its torch form, ShardedRenderer(planes=...) the HIP one) --
up to 68 bytes per pixel instead of 24.
"""
import torch
import torch.distributed as dist

from . import capi

BYTES_PER_PIXEL = 8          # 3 (Color24) + 4 (float z) + 1 (sample count)
BYTES_PER_PIXEL_LINEAR = 24  # the 8-byte record + the linear plane's 3 floats + 4 zero bytes (ShardedRenderer(linear=True))


def tile_grid(width, height, tile_w=32, tile_h=8):
    tiles_x = (width + tile_w - 1) // tile_w
    tiles_y = (height + tile_h - 1) // tile_h
    return tiles_x, tiles_y, tiles_x * tiles_y


def tiles_of_rank(rank, world, n_tiles):
    return torch.arange(rank, n_tiles, world)


def _padded_tiles(rgb, z, cnt, tile_w, tile_h):
    """(H,W,3) u8, (H,W) f32, (H,W) u8  ->  (n_tiles, tile_h, tile_w, 8) u8 view-copy"""
    h, w = z.shape
    tx, ty, _ = tile_grid(w, h, tile_w, tile_h)
    ph, pw = ty * tile_h, tx * tile_w
    px = torch.zeros((ph, pw, BYTES_PER_PIXEL), dtype=torch.uint8, device=z.device)
    px[:h, :w, 0:3] = rgb
    px[:h, :w, 3:7] = z.contiguous().view(torch.uint8).reshape(h, w, 4)
    px[:h, :w, 7] = cnt
    return px.reshape(ty, tile_h, tx, tile_w, BYTES_PER_PIXEL).permute(0, 2, 1, 3, 4).reshape(tx * ty, tile_h, tile_w, BYTES_PER_PIXEL)


def pack_own_tiles(rgb, z, cnt, rank, world, tile_w=32, tile_h=8):
    """Compact buffer of this rank's tiles, padded to the per-rank maximum so that every rank
    contributes the same number of bytes to the all-gather."""
    tiles = _padded_tiles(rgb, z, cnt, tile_w, tile_h)
    n = tiles.shape[0]
    per_rank = (n + world - 1) // world
    out = torch.zeros((per_rank, tile_h, tile_w, BYTES_PER_PIXEL), dtype=torch.uint8, device=z.device)
    mine = tiles[rank::world]
    out[: mine.shape[0]] = mine
    return out.contiguous()


def unpack_gathered(gathered, width, height, world, tile_w=32, tile_h=8):
    """gathered: (world, per_rank, tile_h, tile_w, 8) u8 -> rgb (H,W,3) u8, z (H,W) f32, cnt (H,W) u8"""
    tx, ty, n = tile_grid(width, height, tile_w, tile_h)
    tiles = torch.zeros((n, tile_h, tile_w, BYTES_PER_PIXEL), dtype=torch.uint8, device=gathered.device)
    for r in range(world):
        k = len(range(r, n, world))
        tiles[r::world] = gathered[r, :k]
    px = tiles.reshape(ty, tx, tile_h, tile_w, BYTES_PER_PIXEL).permute(0, 2, 1, 3, 4).reshape(ty * tile_h, tx * tile_w, BYTES_PER_PIXEL)
    px = px[:height, :width]
    rgb = px[..., 0:3].contiguous()
    z = px[..., 3:7].contiguous().view(torch.float32).reshape(height, width)
    cnt = px[..., 7].contiguous()
    return rgb, z, cnt


def gather_frame(rgb, z, cnt, rank, world, tile_w=32, tile_h=8):
    """All-gather the finished tiles; every rank returns the complete frame."""
    h, w = z.shape
    if world == 1:
        return rgb, z, cnt
    mine = pack_own_tiles(rgb, z, cnt, rank, world, tile_w, tile_h)
    gathered = torch.empty((world * mine.shape[0],) + tuple(mine.shape[1:]), dtype=torch.uint8, device=mine.device)
    dist.all_gather_into_tensor(gathered, mine)          # rank r's tiles land in rows [r*per_rank, (r+1)*per_rank)
    return unpack_gathered(gathered.reshape((world,) + tuple(mine.shape)), w, h, world, tile_w, tile_h)


# ---- the packed planes format (include/rt_mi355x.h, "packed planes") in torch: the yardstick of the HIP side ----------------
PLANE_SECTIONS = ("normal", "albedo", "alpha", "object_id", "variance")     # the sections behind the records, in buffer order
PLANE_BYTES = {"linear": 12, "normal": 12, "albedo": 12, "alpha": 4, "object_id": 4, "variance": 12}
ALL_PLANES = ("linear",) + PLANE_SECTIONS


def planes_layout(width, height, world, planes=(), tile_w=32, tile_h=8):
    """(bytes of one contribution, tiles per rank, {section: byte offset or None}) for `world` ranks: every section holds
    per_rank * tile_w * tile_h slots whichever rank writes it; the total is rounded up to 16 bytes."""
    for name in planes:
        PLANE_BYTES[name]                   # KeyError: no such plane
    _, _, n = tile_grid(width, height, tile_w, tile_h)
    per_rank = (n + world - 1) // world
    slots = per_rank * tile_w * tile_h
    off = {"records": 0}
    at = slots * (BYTES_PER_PIXEL_LINEAR if "linear" in planes else BYTES_PER_PIXEL)
    for name in PLANE_SECTIONS:
        off[name] = at if name in planes else None
        if name in planes:
            at += slots * PLANE_BYTES[name]
    return (at + 15) // 16 * 16, per_rank, off


def _bytes_of(plane, h, w):
    """an (H, W) or (H, W, C) plane as (H, W, bytes per pixel) uint8"""
    t = torch.as_tensor(plane).contiguous()
    return t.view(torch.uint8).reshape(h, w, -1)


def _walk_section(px, rank, world, tile_w, tile_h):
    """(H, W, B) u8 -> (per_rank * tile_h * tile_w * B,) u8: this rank's tiles in walk order, zero where no pixel is"""
    h, w, b = px.shape
    tx, ty, n = tile_grid(w, h, tile_w, tile_h)
    pad = torch.zeros((ty * tile_h, tx * tile_w, b), dtype=torch.uint8, device=px.device)
    pad[:h, :w] = px
    tiles = pad.reshape(ty, tile_h, tx, tile_w, b).permute(0, 2, 1, 3, 4).reshape(n, tile_h, tile_w, b)
    per_rank = (n + world - 1) // world
    out = torch.zeros((per_rank, tile_h, tile_w, b), dtype=torch.uint8, device=px.device)
    mine = tiles[rank::world]
    out[: mine.shape[0]] = mine
    return out.reshape(-1)


def pack_own_planes(frame, rank, world, planes=(), tile_w=32, tile_h=8):
    """One rank's contribution in the packed planes format, as a flat uint8 tensor: `frame` is a dict keyed like
    Scene.render_outputs ("rgb", "z", "count" and the names in `planes`; arrays or tensors, CPU or GPU) holding the whole
    frame, of which this rank's tiles rank, rank + world, ... are taken.  Exactly the bytes
    rt_render_tiles_packed_outputs_device writes for TileRange(tile_w, tile_h, rank, world)."""
    z = torch.as_tensor(frame["z"])
    h, w = z.shape
    nbytes, _, off = planes_layout(w, h, world, planes, tile_w, tile_h)
    rec = [_bytes_of(frame["rgb"], h, w), _bytes_of(z, h, w), _bytes_of(frame["count"], h, w)]
    if "linear" in planes:
        rec += [_bytes_of(frame["linear"], h, w), torch.zeros((h, w, 4), dtype=torch.uint8, device=z.device)]
    out = torch.zeros(nbytes, dtype=torch.uint8, device=z.device)
    sec = _walk_section(torch.cat(rec, 2), rank, world, tile_w, tile_h)
    out[: sec.numel()] = sec
    for name in PLANE_SECTIONS:
        if name in planes:
            sec = _walk_section(_bytes_of(frame[name], h, w), rank, world, tile_w, tile_h)
            out[off[name]: off[name] + sec.numel()] = sec
    return out


def unpack_gathered_planes(gathered, width, height, world, planes=(), tile_w=32, tile_h=8):
    """gathered: the contributions of `world` ranks end to end (uint8, world * bytes values in any shape) -> the frame as a
    dict of tensors keyed like Scene.render_outputs: rgb (H, W, 3) u8, z (H, W) f32, count (H, W) u8 and the planes."""
    nbytes, per_rank, off = planes_layout(width, height, world, planes, tile_w, tile_h)
    gathered = gathered.reshape(world, nbytes)
    tx, ty, n = tile_grid(width, height, tile_w, tile_h)

    def image(offset, b):
        """the section at `offset` with b bytes per slot, of every rank -> (H, W, b) u8"""
        sec = gathered[:, offset: offset + per_rank * tile_h * tile_w * b].reshape(world, per_rank, tile_h, tile_w, b)
        tiles = torch.zeros((n, tile_h, tile_w, b), dtype=torch.uint8, device=gathered.device)
        for r in range(world):
            k = len(range(r, n, world))
            tiles[r::world] = sec[r, :k]
        px = tiles.reshape(ty, tx, tile_h, tile_w, b).permute(0, 2, 1, 3, 4).reshape(ty * tile_h, tx * tile_w, b)
        return px[:height, :width]

    linear = "linear" in planes
    px = image(0, BYTES_PER_PIXEL_LINEAR if linear else BYTES_PER_PIXEL)
    out = {"rgb": px[..., 0:3].contiguous(), "z": px[..., 3:7].contiguous().view(torch.float32).reshape(height, width),
           "count": px[..., 7].contiguous()}
    if linear:
        out["linear"] = px[..., 8:20].contiguous().view(torch.float32).reshape(height, width, 3)
    for name in PLANE_SECTIONS:
        if name in planes:
            v = image(off[name], PLANE_BYTES[name]).contiguous()
            if name == "object_id":
                out[name] = v.view(torch.int32).reshape(height, width)
            elif name == "alpha":
                out[name] = v.view(torch.float32).reshape(height, width)
            else:
                out[name] = v.view(torch.float32).reshape(height, width, 3)
    return out


class ShardedRenderer:
    """One process per GPU: this rank's tiles are rendered straight into the buffer it contributes to the
    all-gather (rt_render_tiles_packed_device: k_resolve writes the 8-byte pixel records tile by tile), ONE
    all_gather_into_tensor moves them (RCCL over xGMI), and one small HIP kernel (rt_tiles_unpack_device)
    un-interleaves the gathered tiles into the RenderImage planes -- no Python-side packing in the step.
    `gather_ms` collects, per step, the time from the end of this rank's render to the finished frame.
    linear=True: the frame also carries the linear (pre-gamma) float RGB plane `lin` (H, W, 3): the records grow to 24 bytes
    (still one all-gather) and step() returns (rgb, z, cnt, lin) as its frame.
    planes=(names of Scene.render_outputs' planes: linear, normal, albedo, alpha, object_id, variance): the frame carries them
    too.  The exchange is the packed planes format of the header -- the records plus one section per plane, rendered in place
    (rt_render_tiles_packed_outputs_device), moved by the same ONE all-gather, un-interleaved by one HIP kernel
    (rt_tiles_unpack_outputs_device) -- and step() returns (stats, frame) with frame a dict of device tensors keyed like
    render_outputs: "rgb", "z", "count" and the planes.  With one rank nothing is packed: rt_render_tiles_outputs_device
    writes the planes directly.
    denoise=True: implies the six planes Scene.render_denoised(variance=True) renders; after the un-interleave every rank runs
    the variance-guided denoiser (capi.denoise_device, gamma the render's, denoise_kw its other keywords) on this renderer's
    stream and the frame gains "denoised" (float32 (H, W, 3)) and "denoised_rgb" (uint8 (H, W, 3)).
    What else follows a frame is the caller's, on `sr.stream` with the returned tensors' data_ptr()s: temporal accumulation
    (capi.History.accumulate_device), motion vectors (capi.motion_device -- the motion plane is a function of z and object_id,
    so it needs no transport: compute it after the step), bloom (capi.Bloom.apply_device -- like tone mapping it works on the
    gathered frame, so nothing of it is transported) and tone mapping (capi.Exposure.tonemap_device).  Motion blur
    (capi.MotionBlur.apply_device) is one more of these post stages: it runs after the exchange on the gathered linear, motion and
    z planes, ahead of bloom, and nothing of it is transported.  Depth of field (capi.DepthOfField.apply_device) likewise: render
    with a camera whose dof is 0 and defocus the gathered linear plane from the gathered z after the un-interleave, ahead of
    motion blur; nothing of it is exchanged.
    With planes=None and denoise=False the renderer is what it was: the same bytes exchanged, a tuple as the frame."""

    def __init__(self, scene, cam, params, rank, world, device_index, tile_w=32, tile_h=8, host_gather=False, linear=False,
                 planes=None, denoise=False, denoise_kw=None):
        self.scene, self.cam, self.params = scene, cam, params
        self.host_gather = host_gather          # gather over CPU tensors (gloo rehearsal on one GPU)
        self.rank, self.world, self.device_index = rank, world, device_index
        self.tile_w, self.tile_h = tile_w, tile_h
        dev = torch.device("cuda", device_index)
        h, w = cam.height, cam.width
        self.rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device=dev)
        self.z = torch.zeros((h, w), dtype=torch.float32, device=dev)
        self.cnt = torch.zeros((h, w), dtype=torch.uint8, device=dev)
        self.linear = linear
        self.lin = torch.zeros((h, w, 3), dtype=torch.float32, device=dev) if linear else None
        bpp = BYTES_PER_PIXEL_LINEAR if linear else BYTES_PER_PIXEL
        _, _, n = tile_grid(w, h, tile_w, tile_h)
        self.per_rank = (n + world - 1) // world
        self.denoise, self.denoise_kw = denoise, dict(denoise_kw or {})
        if denoise:
            planes = ALL_PLANES
        if planes is not None and set(planes) - set(ALL_PLANES):
            raise KeyError(f"no such plane: {sorted(set(planes) - set(ALL_PLANES))[0]!r}")
        # the planes in the format's order, whatever order they were named in (linear=True names one of them)
        self.planes = None if planes is None else tuple(k for k in ALL_PLANES if k in planes or (linear and k == "linear"))
        if self.planes is not None:
            self.frame = {"rgb": self.rgb, "z": self.z, "count": self.cnt}
            for name in self.planes:
                shape, dtype = ((h, w), torch.int32 if name == "object_id" else torch.float32) if PLANE_BYTES[name] == 4 else ((h, w, 3), torch.float32)
                self.frame[name] = torch.zeros(shape, dtype=dtype, device=dev)
            if "linear" in self.planes:
                self.lin = self.frame["linear"]
            if denoise:
                self.frame["denoised"] = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
                self.frame["denoised_rgb"] = torch.zeros((h, w, 3), dtype=torch.uint8, device=dev)
            nbytes = planes_layout(w, h, world, self.planes, tile_w, tile_h)[0]
            # flat contributions: the sections have different slot sizes
            self.packed = torch.zeros(nbytes if world > 1 else 0, dtype=torch.uint8, device=dev)
            self.gathered = torch.zeros(world * nbytes if world > 1 else 0, dtype=torch.uint8, device=dev)
        else:
            # ranks whose share is one tile short leave the last slot zero: every rank contributes the same bytes
            self.packed = torch.zeros((self.per_rank, tile_h, tile_w, bpp), dtype=torch.uint8, device=dev)
            self.gathered = torch.zeros((world * self.per_rank, tile_h, tile_w, bpp), dtype=torch.uint8, device=dev)
        self.gather_ms = []
        # everything of a step -- render, all-gather, un-interleave -- is ordered on ONE explicit stream (torch's legacy
        # default stream has handle 0, which the C ABI reads as "the library's own stream": not ordered with ours)
        self.stream = torch.cuda.Stream(device=dev)

    def _stream(self):
        return self.stream.cuda_stream

    def render_own_tiles(self, want_stats=True, sync=True):
        """this rank's tiles into the image planes (single-GPU path, and the profiling leg of bench.py)"""
        tiles = capi.TileRange(self.tile_w, self.tile_h, self.rank, self.world)
        return self.scene.render_tiles_device(self.cam, self.params, tiles, self.device_index, self.rgb.data_ptr(),
                                              self.z.data_ptr(), self.cnt.data_ptr(), stream=self._stream(), sync=sync,
                                              want_stats=want_stats, linear_ptr=self.lin.data_ptr() if self.linear else None)

    def _plane_ptrs(self):
        return {name + "_ptr": self.frame[name].data_ptr() for name in self.planes}

    def render_own_planes(self, want_stats=True, sync=True):
        """planes=...: this rank's tiles with their planes straight into the image-sized tensors (the single-GPU path)"""
        tiles = capi.TileRange(self.tile_w, self.tile_h, self.rank, self.world)
        return self.scene.render_tiles_outputs_device(self.cam, self.params, tiles, self.device_index, self.rgb.data_ptr(),
                                                      self.z.data_ptr(), self.cnt.data_ptr(), stream=self._stream(), sync=sync,
                                                      want_stats=want_stats, **self._plane_ptrs())

    def render_own_planes_packed(self, want_stats=True, sync=True):
        """planes=...: this rank's contribution in the packed planes format"""
        tiles = capi.TileRange(self.tile_w, self.tile_h, self.rank, self.world)
        return self.scene.render_tiles_packed_outputs_device(self.cam, self.params, tiles, self.device_index, self.packed.data_ptr(),
                                                             self.packed.numel(), stream=self._stream(), sync=sync,
                                                             want_stats=want_stats, planes=self.planes)

    def _denoise(self, sync):
        f = self.frame
        kw = dict({"gamma": self.params.gamma}, **self.denoise_kw)
        capi.denoise_device(self.device_index, self._stream(), self.cam.width, self.cam.height, linear_ptr=f["linear"].data_ptr(),
                            normal_ptr=f["normal"].data_ptr(), albedo_ptr=f["albedo"].data_ptr(), z_ptr=f["z"].data_ptr(),
                            out_ptr=f["denoised"].data_ptr(), object_id_ptr=f["object_id"].data_ptr(),
                            rgb8_ptr=f["denoised_rgb"].data_ptr(), sync=sync, variance_ptr=f["variance"].data_ptr(), **kw)

    def render_own_tiles_packed(self, want_stats=True, sync=True):
        tiles = capi.TileRange(self.tile_w, self.tile_h, self.rank, self.world)
        return self.scene.render_tiles_packed_device(self.cam, self.params, tiles, self.device_index, self.packed.data_ptr(),
                                                     self.packed.numel(), stream=self._stream(), sync=sync, want_stats=want_stats,
                                                     linear=self.linear)

    def _frame(self):
        if self.planes is not None:
            return self.frame
        return (self.rgb, self.z, self.cnt, self.lin) if self.linear else (self.rgb, self.z, self.cnt)

    def step(self, sync=True):
        """One frame.  sync=True: the call returns with the finished frame and this rank's statistics (the host waits for the
        render before it starts the exchange).  sync=False: everything -- render, all-gather, un-interleave -- is only ENQUEUED
        on this renderer's stream (the library orders a frame behind the one before it on the GPU, the collective follows in
        stream order); no statistics, no host round trip between frames: call finish() before reading the frame.  The first
        frame of a renderer should be a synchronous one (it sizes the queues from measurement; an asynchronous render
        without history takes worst-case queues)."""
        with_planes = self.planes is not None
        if self.world == 1:
            st = self.render_own_planes(want_stats=sync, sync=sync) if with_planes else self.render_own_tiles(want_stats=sync, sync=sync)
            if self.denoise:
                self._denoise(sync)
            self.gather_ms.append(0.0)
            return (st if sync else None), self._frame()
        import time
        with torch.cuda.stream(self.stream):
            # sync: this rank's tiles are final
            st = (self.render_own_planes_packed if with_planes else self.render_own_tiles_packed)(want_stats=sync, sync=sync)
            t0 = time.perf_counter()
            if self.host_gather:
                self.stream.synchronize()
                mine = self.packed.cpu()
                gathered = torch.empty((self.world * mine.shape[0],) + tuple(mine.shape[1:]), dtype=torch.uint8)
                dist.all_gather_into_tensor(gathered, mine)
                self.gathered.copy_(gathered)
            else:
                dist.all_gather_into_tensor(self.gathered, self.packed)     # rank r's tiles land in rows [r*per_rank, (r+1)*per_rank)
            if with_planes:
                capi.tiles_unpack_outputs_device(self.device_index, self._stream(), self.gathered.data_ptr(), self.world, self.per_rank,
                                                 self.cam.width, self.cam.height, self.tile_w, self.tile_h,
                                                 self.rgb.data_ptr(), self.z.data_ptr(), self.cnt.data_ptr(),
                                                 planes=self.planes, **self._plane_ptrs())
                if self.denoise:
                    self._denoise(False)
            else:
                capi.tiles_unpack_device(self.device_index, self._stream(), self.gathered.data_ptr(), self.world, self.per_rank,
                                         self.cam.width, self.cam.height, self.tile_w, self.tile_h,
                                         self.rgb.data_ptr(), self.z.data_ptr(), self.cnt.data_ptr(),
                                         linear_ptr=self.lin.data_ptr() if self.linear else None)
            if sync:
                self.stream.synchronize()
        if sync:
            self.gather_ms.append((time.perf_counter() - t0) * 1e3)
        return (st if sync else None), self._frame()

    def finish(self):
        """wait for the frames enqueued with step(sync=False) and collect their verdict (raises if a queue overflowed)"""
        self.stream.synchronize()
        self.scene.render_check(self.device_index)
