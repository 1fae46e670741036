"""The packed planes format on the GPU (include/rt_mi355x.h, "packed planes"): rt_render_tiles_packed_outputs_device writes a
rank's contribution, rt_tiles_unpack_outputs_device (k_unpack_planes) un-interleaves the gathered ones.  Ranks render in turn
into one "gathered" tensor on one GPU -- no collective.  Everything is held byte for byte to ONE reproducible reference frame
(Scene.render_outputs with all six planes) through the torch helpers of raytracing_folder_amd/dist.py, which
tests/test_dist_planes.py checks on the CPU."""
import numpy as np
import pytest

from raytracing_folder_amd import capi, photons
from raytracing_folder_amd import dist as rtd
from tests import scenes

pytestmark = pytest.mark.gpu

W, H = 100, 37                                                  # 4 x 5 tiles of 32 x 8, ragged right and bottom
ALL = rtd.ALL_PLANES
NINE = ("rgb", "z", "count") + ALL
PAD = dict(min_sample=4, max_sample=8, threshold=1e-3)          # adaptive 4 -> 8 (the variance gate)
BG = (0.25, 0.5, 0.75)
SENT = 0xAB                                                     # what buffers hold before a call: nothing may rely on zeros


@pytest.fixture(scope="module")
def ref():
    """the reproducible Cornell frame of tests/test_linear_output.py at 100 x 37, with every plane"""
    bal = photons.synth_cornell_photon_map(20000, seed=3)
    s, cam = scenes.load_cornell(W, H)
    s.set_environment((0, 0, 0), BG)
    s.set_photons(bal)
    cam.fov = 70.0
    s.set_render_flags(capi.RENDER_REPRODUCIBLE)
    p = capi.default_params(**PAD)
    frame = s.render_outputs(cam, p, planes=ALL)
    assert (frame["object_id"] == -1).any()                     # all-miss pixels
    assert (frame["count"] == 255).any()                        # second-batch pixels
    assert (frame["variance"] > 0).any()
    assert frame["stats"].photon_queries > 0
    return s, cam, p, frame


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _exchange(s, cam, p, world, planes):
    """every rank's contribution rendered in turn into its block of one gathered tensor (pre-filled with SENT)"""
    torch, dev = _torch()
    side = torch.cuda.Stream(device=dev)
    nbytes, per_rank, off = capi.tiles_packed_planes_size(W, H, capi.TileRange(32, 8, 0, world), planes)
    gathered = torch.full((world, nbytes), SENT, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for rank in range(world):
        s.render_tiles_packed_outputs_device(cam, p, capi.TileRange(32, 8, rank, world), 0, gathered[rank].data_ptr(), nbytes,
                                             stream=side.cuda_stream, sync=True, want_stats=False, planes=planes)
    torch.cuda.synchronize()
    return gathered, nbytes, per_rank, off, side


def _empty_planes(fill=SENT):
    torch, dev = _torch()
    t = {"rgb": torch.full((H, W, 3), fill, dtype=torch.uint8, device=dev), "z": torch.full((H, W), 0, dtype=torch.float32, device=dev),
         "count": torch.full((H, W), fill, dtype=torch.uint8, device=dev), "alpha": torch.full((H, W), 0, dtype=torch.float32, device=dev),
         "object_id": torch.full((H, W), 0, dtype=torch.int32, device=dev)}
    for name in ("linear", "normal", "albedo", "variance"):
        t[name] = torch.full((H, W, 3), 0, dtype=torch.float32, device=dev)
    for v in t.values():
        v.view(torch.uint8).fill_(fill)                          # the same sentinel byte in every plane
    return t


def _unpack(gathered, world, per_rank, side, out, planes):
    torch, dev = _torch()
    torch.cuda.synchronize()
    capi.tiles_unpack_outputs_device(0, side.cuda_stream, gathered.data_ptr(), world, per_rank, W, H, 32, 8, out["rgb"].data_ptr(),
                                     out["z"].data_ptr(), out["count"].data_ptr(), planes=planes,
                                     **{k + "_ptr": out[k].data_ptr() for k in ALL})
    torch.cuda.synchronize()


def _assert_same(got, want, names):
    for name in names:
        a = got[name].cpu().numpy() if hasattr(got[name], "cpu") else np.asarray(got[name])
        b = np.asarray(want[name])
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert a.tobytes() == b.tobytes(), f"{name}: {(a != b).sum()} values differ"


def _is_sentinel(t):
    torch, _ = _torch()
    return bool((t.contiguous().view(torch.uint8) == SENT).all())


@pytest.fixture(scope="module")
def exchanged(ref):
    """the world-3 and world-8 exchanges of the reference frame with all six planes, rendered once"""
    s, cam, p, frame = ref
    return {world: _exchange(s, cam, p, world, ALL) for world in (3, 8)}


@pytest.mark.parametrize("world", [3, 8])
def test_contributions_are_the_helpers_bytes_and_unpack_to_the_reference(ref, exchanged, world):
    torch, dev = _torch()
    s, cam, p, frame = ref
    gathered, nbytes, per_rank, off, side = exchanged[world]
    assert nbytes == per_rank * 256 * 68
    host = gathered.cpu().numpy()
    for rank in range(world):
        want = rtd.pack_own_planes(frame, rank, world, ALL).numpy()
        assert want.size == nbytes
        diff = np.flatnonzero(host[rank] != want)
        assert diff.size == 0, f"rank {rank}: {diff.size} bytes differ, the first at {diff[0]}"        # layout, zero slots, short rank
        # the records section: the bytes of the existing 24-byte packed call
        tiles = capi.TileRange(32, 8, rank, world)
        n24, k = capi.tiles_packed_size(W, H, tiles, linear=True)
        old = torch.full((n24,), SENT, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        s.render_tiles_packed_device(cam, p, tiles, 0, old.data_ptr(), n24, stream=side.cuda_stream, sync=True, want_stats=False, linear=True)
        torch.cuda.synchronize()
        assert k in (per_rank, per_rank - 1) and old.cpu().numpy().tobytes() == host[rank, :n24].tobytes()
    out = _empty_planes()
    _unpack(gathered, world, per_rank, side, out, ALL)
    _assert_same(out, frame, NINE)
    # the helpers read the same frame out of the GPU's bytes
    _assert_same(rtd.unpack_gathered_planes(gathered.cpu(), W, H, world, ALL), frame, NINE)


@pytest.mark.parametrize("w,h,tw,th,world,planes", [
    (33, 9, 32, 8, 2, ALL),                         # width no multiple of 4: one pixel per thread; 4 tiles
    (7, 5, 3, 3, 4, ("alpha", "variance")),         # odd tiles: contributions rounded up to 16 bytes, sections only 4-byte aligned
    (1026, 520, 32, 8, 8, ALL),                     # one pixel per thread, more pixels than the grid has threads (grid stride)
    (2048, 1032, 32, 8, 8, ALL),                    # four pixels per thread, more groups than the grid has threads
    (96, 16, 16, 16, 5, ("linear", "object_id")),   # four pixels per thread, ranks without a tile (6 tiles, 5 ranks: 2 per rank)
])
def test_unpack_kernel_on_synthetic_frames(w, h, tw, th, world, planes):
    """k_unpack_planes alone, both instantiations, against the torch helpers: a random frame packed by pack_own_planes on the
    device, un-interleaved by the kernel, compared on the device"""
    torch, dev = _torch()
    g = torch.Generator(device=dev).manual_seed(w * 131 + h)
    f = {"rgb": torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev, generator=g),
         "z": torch.rand((h, w), device=dev, generator=g), "count": torch.randint(0, 256, (h, w), dtype=torch.uint8, device=dev, generator=g),
         "alpha": torch.rand((h, w), device=dev, generator=g),
         "object_id": torch.randint(-1, 1000, (h, w), dtype=torch.int32, device=dev, generator=g)}
    for name in ("linear", "normal", "albedo", "variance"):
        f[name] = torch.rand((h, w, 3), device=dev, generator=g)
    nbytes, per_rank, off = capi.tiles_packed_planes_size(w, h, capi.TileRange(tw, th, 0, world), planes)
    assert (nbytes, per_rank, off) == rtd.planes_layout(w, h, world, planes, tw, th)
    gathered = torch.stack([rtd.pack_own_planes(f, r, world, planes, tw, th) for r in range(world)])
    assert gathered.shape == (world, nbytes)
    out = {k: torch.empty_like(v) for k, v in f.items()}
    for v in out.values():
        v.view(torch.uint8).fill_(SENT)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    capi.tiles_unpack_outputs_device(0, side.cuda_stream, gathered.data_ptr(), world, per_rank, w, h, tw, th, out["rgb"].data_ptr(),
                                     out["z"].data_ptr(), out["count"].data_ptr(), planes=planes,
                                     **{k + "_ptr": out[k].data_ptr() for k in ALL})
    torch.cuda.synchronize()
    for name in NINE:
        if name in ("rgb", "z", "count") + tuple(planes):
            assert torch.equal(out[name].view(torch.uint8), f[name].view(torch.uint8)), name
        else:
            assert _is_sentinel(out[name]), name


def test_masks(ref):
    torch, dev = _torch()
    s, cam, p, frame = ref
    world = 3
    planes = ("alpha", "object_id")
    gathered, nbytes, per_rank, off, side = _exchange(s, cam, p, world, planes)
    assert nbytes == per_rank * 256 * 16 and off["normal"] is None
    host = gathered.cpu().numpy()
    for rank in range(world):
        assert host[rank].tobytes() == rtd.pack_own_planes(frame, rank, world, planes).numpy().tobytes()
    out = _empty_planes()
    _unpack(gathered, world, per_rank, side, out, planes)             # every destination is given, two are in the mask
    _assert_same(out, frame, ("rgb", "z", "count") + planes)
    for name in ("linear", "normal", "albedo", "variance"):
        assert _is_sentinel(out[name]), name
    # {} and {linear}: the existing packed calls, to the byte, and zeros up to the per-rank size
    for planes, linear in (((), False), (("linear",), True)):
        gathered, nbytes, per_rank, off, side = _exchange(s, cam, p, world, planes)
        host = gathered.cpu().numpy()
        for rank in range(world):
            tiles = capi.TileRange(32, 8, rank, world)
            n_old, k = capi.tiles_packed_size(W, H, tiles, linear=linear)
            old = torch.full((n_old,), SENT, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            s.render_tiles_packed_device(cam, p, tiles, 0, old.data_ptr(), n_old, stream=side.cuda_stream, sync=True, want_stats=False,
                                         linear=linear)
            torch.cuda.synchronize()
            assert host[rank, :n_old].tobytes() == old.cpu().numpy().tobytes()
            assert (host[rank, n_old:] == 0).all() and (n_old == nbytes) == (k == per_rank)
            assert host[rank].tobytes() == rtd.pack_own_planes(frame, rank, world, planes).numpy().tobytes()
        out = _empty_planes()
        _unpack(gathered, world, per_rank, side, out, planes)
        _assert_same(out, frame, ("rgb", "z", "count") + planes)
        assert _is_sentinel(out["normal"]) and (linear or _is_sentinel(out["linear"]))


def test_chunking_moves_no_byte(ref, exchanged, monkeypatch):
    s, cam, p, frame = ref
    # 8192 samples = 1024 pixels = 4 tiles a chunk: two chunks for a rank of 7 tiles, so k_features and k_resolve write into
    # the sections more than once per call
    monkeypatch.setenv("RT_CHUNK_SAMPLES", "8192")
    gathered = _exchange(s, cam, p, 3, ALL)[0]
    assert gathered.cpu().numpy().tobytes() == exchanged[3][0].cpu().numpy().tobytes()


def test_sharded_renderer_on_one_rank(ref):
    s, cam, p, frame = ref
    sr = rtd.ShardedRenderer(s, cam, p, 0, 1, 0, planes=ALL)
    st, got = sr.step(sync=True)
    assert isinstance(got, dict) and set(got) == set(NINE) and st.photon_queries > 0
    _assert_same(got, frame, NINE)
    # asynchronous: only enqueued, the same frame after finish()
    import torch
    for v in got.values():
        v.zero_()
    torch.cuda.synchronize()
    st, got = sr.step(sync=False)
    assert st is None
    sr.finish()
    _assert_same(got, frame, NINE)
    want = s.render_denoised(cam, p, variance=True)
    st, got = rtd.ShardedRenderer(s, cam, p, 0, 1, 0, denoise=True).step(sync=True)
    assert set(got) == set(NINE) | {"denoised", "denoised_rgb"}
    _assert_same(got, want, NINE + ("denoised", "denoised_rgb"))
    assert (want["denoised"] != want["linear"]).any()
    # without planes the renderer is what it was
    st, got = rtd.ShardedRenderer(s, cam, p, 0, 1, 0).step(sync=True)
    assert isinstance(got, tuple) and len(got) == 3


def test_the_post_stack_on_an_exchanged_frame(ref, exchanged):
    torch, dev = _torch()
    s, cam, p, frame = ref
    gathered, nbytes, per_rank, off, side = exchanged[3]
    got = _empty_planes()
    _unpack(gathered, 3, per_rank, side, got, ALL)
    single = {k: torch.from_numpy(np.ascontiguousarray(frame[k])).to(dev) for k in NINE}
    nodes = s.get_nodes()
    res = []
    for f in (got, single):
        den = torch.full((H, W, 3), 0, dtype=torch.float32, device=dev)
        den8 = torch.full((H, W, 3), 0, dtype=torch.uint8, device=dev)
        mot = torch.full((H, W, 3), 0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        capi.denoise_device(0, side.cuda_stream, W, H, linear_ptr=f["linear"].data_ptr(), normal_ptr=f["normal"].data_ptr(),
                            albedo_ptr=f["albedo"].data_ptr(), z_ptr=f["z"].data_ptr(), out_ptr=den.data_ptr(),
                            object_id_ptr=f["object_id"].data_ptr(), rgb8_ptr=den8.data_ptr(), sync=True,
                            variance_ptr=f["variance"].data_ptr(), gamma=p.gamma)
        capi.motion_device(0, side.cuda_stream, cam, cam, nodes, None, z_ptr=f["z"].data_ptr(), object_id_ptr=f["object_id"].data_ptr(),
                           motion_ptr=mot.data_ptr(), sync=True)
        torch.cuda.synchronize()
        res.append({"denoised": den.cpu().numpy(), "denoised_rgb": den8.cpu().numpy(), "motion": mot.cpu().numpy()})
    _assert_same(res[0], res[1], ("denoised", "denoised_rgb", "motion"))
    assert (res[0]["denoised"] != frame["linear"]).any() and (res[0]["motion"][..., 2] > 0).any()


def test_argument_errors_leave_the_outputs_alone(ref, exchanged):
    torch, dev = _torch()
    s, cam, p, frame = ref
    gathered, nbytes, per_rank, off, side = exchanged[3]
    buf = torch.full((nbytes,), SENT, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    tiles = capi.TileRange(32, 8, 2, 3)                              # the short rank: its own tiles would fit a smaller buffer
    with pytest.raises(capi.RtError) as e:
        s.render_tiles_packed_outputs_device(cam, p, tiles, 0, buf.data_ptr(), nbytes - 1, stream=side.cuda_stream, planes=ALL)
    assert e.value.status == -1
    import ctypes as C
    L = capi.lib()
    assert L.rt_render_tiles_packed_outputs_device(s._h, C.byref(cam), C.byref(p), C.byref(tiles), 0, C.c_void_p(side.cuda_stream),
                                                   C.c_void_p(buf.data_ptr()), nbytes, 64 | 63, 1, None) == -1
    torch.cuda.synchronize()
    assert _is_sentinel(buf)
    out = _empty_planes()
    ptrs = {k + "_ptr": out[k].data_ptr() for k in ALL}
    args = (0, side.cuda_stream, gathered.data_ptr(), 3, per_rank, W, H, 32, 8, out["rgb"].data_ptr(), out["z"].data_ptr(), out["count"].data_ptr())
    for missing in ("variance", "normal", "linear"):
        with pytest.raises(capi.RtError) as e:
            capi.tiles_unpack_outputs_device(*args, planes=ALL, **dict(ptrs, **{missing + "_ptr": None}))
        assert e.value.status == -1, missing
    o = capi.Outputs(rgb8=out["rgb"].data_ptr(), z=out["z"].data_ptr(), count=out["count"].data_ptr(),
                     **{capi.OUTPUT_PLANES[k][0]: out[k].data_ptr() for k in ALL if k != "variance"})
    assert L.rt_tiles_unpack_outputs_device(0, C.c_void_p(side.cuda_stream), C.c_void_p(gathered.data_ptr()), 3, per_rank, W, H, 32, 8,
                                            128, C.byref(o), C.c_void_p(out["variance"].data_ptr())) == -1
    # too few tiles per rank for the frame
    assert L.rt_tiles_unpack_outputs_device(0, C.c_void_p(side.cuda_stream), C.c_void_p(gathered.data_ptr()), 3, per_rank - 1, W, H, 32, 8,
                                            63, C.byref(o), C.c_void_p(out["variance"].data_ptr())) == -1
    torch.cuda.synchronize()
    for name in NINE:
        assert _is_sentinel(out[name]), name
