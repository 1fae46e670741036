"""ctypes binding of librt_mi355x.so (the C ABI declared in include/rt_mi355x.h): the module everything imports.  abi.py holds the
ABI itself (records, structs, the signature table, lib()), stages.py the image-space stages; both are imported here whole, and the
scene side, the photon, image and tile helpers follow.

The render entry points run ONLY on the HIP kernels; when the library or a gfx950 device is
missing they raise -- there is no CPU fallback in this package.
"""
from .abi import *  # noqa: F401,F403
from .abi import _Handle, _c, _check, _p, _stream_handle
from .stages import *  # noqa: F401,F403

_denoise = denoise       # for Scene.render_temporal, whose `denoise` argument hides the function


def device_bvh_cost(nodes, root_ref):
    """rt_device_bvh_cost, the host mirror of k_bvh_cost (no GPU): (cost, degenerate) of DEVBVHNODE records and their root ref"""
    nodes = _c(nodes, DEVBVHNODE)
    cost, flags = C.c_double(0.0), C.c_uint32(0)
    _check(lib().rt_device_bvh_cost(_p(nodes), len(nodes), int(root_ref), C.byref(cost), C.byref(flags)))
    return cost.value, bool(flags.value & MESH_QUALITY_DEGENERATE)


def device_lbvh_build(v, f):
    """rt_device_lbvh_build, the host mirror of the device tree build (no GPU): (DeviceBvhInfo, DEVBVHNODE records, face of every
    triangle slot) of bare triangles, in the form of Scene.mesh_device_read's info / nodes / slot_face"""
    v, f = _c(v, np.float32).reshape(-1, 3), _c(f, np.uint32).reshape(-1, 3)
    info = DeviceBvhInfo(struct_size=C.sizeof(DeviceBvhInfo))
    _check(lib().rt_device_lbvh_build(_p(v), len(v), _p(f), len(f), C.byref(info), None, 0, None, 0))
    nodes, slot_face = np.zeros(info.n_nodes, DEVBVHNODE), np.zeros(info.n_slots, np.uint32)
    _check(lib().rt_device_lbvh_build(_p(v), len(v), _p(f), len(f), C.byref(info), _p(nodes), len(nodes), _p(slot_face), len(slot_face)))
    return info, nodes, slot_face


def mesh_smooth_normals(v, f, fn=None, vn=None):
    """rt_mesh_smooth_normals, the host mirror of k_mesh_normals (no GPU): the smooth normals of positions v under faces f and
    normal indices fn (None: f), float32 (nvn, 3).  vn holds the stored values, which a normal without a corner or without a
    direction keeps (it is not modified); None: as many normals as vertices, stored values 0."""
    v, f = _c(v, np.float32).reshape(-1, 3), _c(f, np.uint32).reshape(-1, 3)
    fn = _c(fn, np.uint32).reshape(-1, 3) if fn is not None else None
    out = np.array(vn, np.float32).reshape(-1, 3) if vn is not None else np.zeros((len(v), 3), np.float32)
    _check(lib().rt_mesh_smooth_normals(_p(v), len(v), _p(f), _p(fn), len(f), _p(out), len(out)))
    return out


def mesh_skin(v_rest, bone_index, weight, bones):
    """rt_mesh_skin, the host mirror of k_mesh_pose's skinning (no GPU): the posed positions, float32 (nv, 3), of rest positions v_rest under
    four influences a vertex -- bone_index uint16 (nv, 4), weight float32 (nv, 4) -- and the pose bones, float32 (n_bones, 3, 4)"""
    v = _c(v_rest, np.float32).reshape(-1, 3)
    idx, w = _c(bone_index, np.uint16).reshape(-1, 4), _c(weight, np.float32).reshape(-1, 4)
    bones = _c(bones, np.float32).reshape(-1, 3, 4)
    if not len(idx) == len(w) == len(v):
        raise ValueError(f"mesh_skin: {len(v)} vertices, {len(idx)} index rows, {len(w)} weight rows")
    out = np.zeros((len(v), 3), np.float32)
    _check(lib().rt_mesh_skin(_p(v), len(v), _p(idx), _p(w), _p(bones), len(bones), _p(out)))
    return out


def mesh_morph(v_base, deltas, weights):
    """rt_mesh_morph, the host mirror of k_mesh_pose's morph targets (no GPU): the morphed positions, float32 (nv, 3), of base positions v_base under
    the targets deltas, float32 (n_targets, nv, 3), and one weight a target -- a zero weight skips its target"""
    v = _c(v_base, np.float32).reshape(-1, 3)
    w = _c(weights, np.float32).reshape(-1)
    d = _c(deltas, np.float32).reshape(-1, len(v), 3)
    if len(d) != len(w):
        raise ValueError(f"mesh_morph: {len(d)} targets, {len(w)} weights")
    out = np.zeros((len(v), 3), np.float32)
    _check(lib().rt_mesh_morph(_p(v), len(v), _p(d), len(d), _p(w), _p(out)))
    return out


def default_params(**kw):
    p = Params()
    lib().rt_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def device_count():
    return lib().rt_device_count()


def bvh_build(v, f, max_per_leaf=4):
    v = _c(v, np.float32).reshape(-1, 3)
    f = _c(f, np.uint32).reshape(-1, 3)
    nodes = np.zeros(2 * len(f) + 2, BVHNODE)
    el = np.zeros(len(f), np.uint32)
    n = C.c_int32()
    _check(lib().rt_bvh_build(_p(v), len(v), _p(f), len(f), int(max_per_leaf), _p(nodes), C.byref(n), _p(el)))
    return nodes[:n.value].copy(), el


def image_read_rgb(path):
    w, h = C.c_int32(), C.c_int32()
    _check(lib().rt_image_read_rgb(os.fsencode(path), C.byref(w), C.byref(h), None, 0))
    rgb = np.zeros((h.value, w.value, 3), np.uint8)
    _check(lib().rt_image_read_rgb(os.fsencode(path), C.byref(w), C.byref(h), _p(rgb), rgb.size))
    return rgb


def image_write_png(path, data):
    data = np.ascontiguousarray(data, np.uint8)
    comps = 1 if data.ndim == 2 else data.shape[2]
    _check(lib().rt_image_write_png(os.fsencode(path), _p(data), data.shape[1], data.shape[0], comps))


def zbuffer_image(z):
    """RenderImage::ComputeZBufferImage (scene.h:591-613) of a float z buffer (h, w)."""
    z = np.ascontiguousarray(z, np.float32)
    out = np.zeros(z.shape, np.uint8)
    _check(lib().rt_image_zbuffer(_p(z), z.shape[1], z.shape[0], _p(out)))
    return out


def sample_count_image(cnt):
    """RenderImage::ComputeSampleCountImage (scene.h:615-637): (image, smax)."""
    cnt = np.ascontiguousarray(cnt, np.uint8)
    out = np.zeros(cnt.shape, np.uint8)
    smax = C.c_int32()
    _check(lib().rt_image_sample_count(_p(cnt), cnt.shape[1], cnt.shape[0], _p(out), C.byref(smax)))
    return out, smax.value


def tiles_packed_size(width, height, tiles, linear=False):
    """(bytes, tiles) of this call's packed records: 8 bytes per tile pixel, 24 with the linear plane (linear=True)"""
    nbytes, n = C.c_uint64(), C.c_int32()
    _check(lib().rt_tiles_packed_size(int(width), int(height), C.byref(tiles), C.byref(nbytes), C.byref(n)))
    return nbytes.value * (3 if linear else 1), n.value


def tiles_unpack_device(device, stream, gathered_ptr, world, tiles_per_rank, width, height, tile_w, tile_h, rgb_ptr, z_ptr, cnt_ptr,
                        linear_ptr=None):
    """gathered packed tiles of `world` ranks -> RenderImage planes, one HIP kernel on `stream` (an explicit stream's
    handle; None = the null stream of the device).  linear_ptr: the records are 24-byte ones and the linear plane
    (float32 (H, W, 3)) is written there too."""
    args = (device, _stream_handle(stream), gathered_ptr, int(world), int(tiles_per_rank), int(width), int(height), int(tile_w),
            int(tile_h), rgb_ptr, z_ptr, cnt_ptr)
    if linear_ptr is None:
        _check(lib().rt_tiles_unpack_device(*args))
    else:
        _check(lib().rt_tiles_unpack_linear_device(*args, linear_ptr))


def plane_mask(planes):
    """the RT_PLANE_* mask of plane names (those of Scene.render_outputs)"""
    mask = 0
    for name in planes:
        mask |= PLANE_BITS[name]            # KeyError: no such plane
    return mask


def tiles_packed_planes_size(width, height, tiles, planes=()):
    """One rank's contribution in the packed planes format (rt_tiles_packed_planes_size): (bytes, tiles per rank, offsets) --
    offsets: section name ("records", then the plane names) -> its byte offset in the contribution, None for a plane that is
    not in `planes`.  Sized by the per-rank tile count of tiles.stride ranks, so neither depends on tiles.first."""
    nbytes, n, off = C.c_uint64(), C.c_int32(), (C.c_uint64 * 6)()
    _check(lib().rt_tiles_packed_planes_size(int(width), int(height), C.byref(tiles), plane_mask(planes), C.byref(nbytes), C.byref(n), off))
    return nbytes.value, n.value, {name: (None if o == 2 ** 64 - 1 else o) for name, o in zip(PACKED_SECTIONS, off)}


def tiles_unpack_outputs_device(device, stream, gathered_ptr, world, tiles_per_rank, width, height, tile_w, tile_h, rgb_ptr, z_ptr, cnt_ptr,
                                planes=None, linear_ptr=None, normal_ptr=None, albedo_ptr=None, alpha_ptr=None, object_id_ptr=None,
                                variance_ptr=None):
    """gathered contributions of `world` ranks in the packed planes format -> image-sized DEVICE planes, one HIP kernel on
    `stream` (as tiles_unpack_device).  planes: the names the contributions were rendered with; None = those whose *_ptr is
    given.  A plane in `planes` without a pointer is refused; a pointer whose plane is not in `planes` is left untouched."""
    ptrs = dict(linear=linear_ptr, normal=normal_ptr, albedo=albedo_ptr, alpha=alpha_ptr, object_id=object_id_ptr, variance=variance_ptr)
    if planes is None:
        planes = [k for k, v in ptrs.items() if v is not None]
    o = Outputs(rgb8=rgb_ptr, z=z_ptr, count=cnt_ptr, rgb_linear=linear_ptr, normal=normal_ptr, albedo=albedo_ptr, alpha=alpha_ptr,
                object_id=object_id_ptr)
    _check(lib().rt_tiles_unpack_outputs_device(device, _stream_handle(stream), gathered_ptr, int(world), int(tiles_per_rank),
                                                int(width), int(height), int(tile_w), int(tile_h), plane_mask(planes), C.byref(o), variance_ptr))


def image_write_pfm(path, rgb):
    """float (H, W, 3) -> PFM (little-endian, scanlines bottom to top)"""
    rgb = np.ascontiguousarray(rgb, np.float32)
    assert rgb.ndim == 3 and rgb.shape[2] == 3
    _check(lib().rt_image_write_pfm(os.fsencode(path), _p(rgb), rgb.shape[1], rgb.shape[0]))


def image_read_pfm(path):
    """a 3-channel PFM -> float32 (H, W, 3), row 0 = top"""
    w, h = C.c_int32(), C.c_int32()
    _check(lib().rt_image_read_pfm(os.fsencode(path), C.byref(w), C.byref(h), None, 0))
    rgb = np.zeros((h.value, w.value, 3), np.float32)
    _check(lib().rt_image_read_pfm(os.fsencode(path), C.byref(w), C.byref(h), _p(rgb), rgb.size))
    return rgb


def image_write_pfm1(path, v):
    """float (H, W) -> one-channel PFM ("Pf", little-endian, scanlines bottom to top)"""
    v = np.ascontiguousarray(v, np.float32)
    assert v.ndim == 2
    _check(lib().rt_image_write_pfm1(os.fsencode(path), _p(v), v.shape[1], v.shape[0]))


def image_read_pfm1(path):
    """a one-channel PFM ("Pf") -> float32 (H, W), row 0 = top"""
    w, h = C.c_int32(), C.c_int32()
    _check(lib().rt_image_read_pfm1(os.fsencode(path), C.byref(w), C.byref(h), None, 0))
    v = np.zeros((h.value, w.value), np.float32)
    _check(lib().rt_image_read_pfm1(os.fsencode(path), C.byref(w), C.byref(h), _p(v), v.size))
    return v


def _copy_camera(cam):
    c = Camera()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(Camera))
    return c


def _pinhole(cam):
    """a copy of `cam` without its lens: what a frame is rendered with when a DepthOfField stage stands in for it"""
    c = _copy_camera(cam)
    c.dof = 0.0
    return c


def identity_map(texture=MAP_NONE):
    m = np.zeros(1, TEXMAP)
    m["texture"] = texture
    m["tm"][0, [0, 4, 8]] = 1
    m["itm"][0, [0, 4, 8]] = 1
    return m


def photons_write_dat(path, photons_1based):
    """the reference's photonmap.dat: records [1..n] of a 1-based photon array, 24 bytes each"""
    a = _c(photons_1based, PHOTON)
    _check(lib().rt_photons_write_dat(str(path).encode(), _p(a), max(0, len(a) - 1)))


def photons_read_dat(path):
    """1-based photon array (entry 0 unused) from a photonmap.dat"""
    n = C.c_uint32()
    _check(lib().rt_photons_read_dat(str(path).encode(), None, 0, C.byref(n)))
    out = np.zeros(n.value + 1, PHOTON)
    _check(lib().rt_photons_read_dat(str(path).encode(), _p(out), len(out), C.byref(n)))
    return out


def photon_balance(photons_1based):
    a = _c(photons_1based, PHOTON).copy()
    out = np.zeros_like(a)
    _check(lib().rt_photon_balance(_p(a), len(a) - 1, _p(out)))
    return out


def photon_unreachable(photons_1based):
    """1-based indices into an UNBALANCED photon array of the photons LocatePhotons cannot reach after balancing"""
    a = _c(photons_1based, PHOTON)
    idx = np.zeros(8, np.uint32)
    n = C.c_uint32()
    _check(lib().rt_photon_unreachable(_p(a), len(a) - 1, _p(idx), 8, C.byref(n)))
    return idx[: n.value].copy()


def photon_unreachable_device(photons_1based, device=0):
    """the same on the GPU (rt_photon_unreachable_device): (sorted 1-based raw indices, exact); exact == False: a median key is not
    unique, only the host function answers"""
    ph = np.ascontiguousarray(photons_1based, PHOTON)
    idx = np.zeros(16, np.uint32)
    cnt, exact = C.c_uint32(), C.c_int32()
    _check(lib().rt_photon_unreachable_device(device, _p(ph), len(ph) - 1, _p(idx), 16, C.byref(cnt), C.byref(exact)))
    return idx[:cnt.value].copy(), bool(exact.value)


class Scene(_Handle):
    """Owns an rt_scene handle."""

    _destroy = "rt_scene_destroy"

    def __init__(self):
        self._h = C.c_void_p()
        _check(lib().rt_scene_create(C.byref(self._h)))
        self._keep = []

    # -- setters -------------------------------------------------------------------------------
    def set_nodes(self, nodes):
        nodes = _c(nodes, NODE)
        _check(lib().rt_scene_set_nodes(self._h, _p(nodes), len(nodes)))

    def set_mesh(self, index, v, f, vn, fn, nodes, elements, vt=None, ft=None):
        v, vn = _c(v, np.float32).reshape(-1, 3), _c(vn, np.float32).reshape(-1, 3)
        f, fn = _c(f, np.uint32).reshape(-1, 3), _c(fn, np.uint32).reshape(-1, 3)
        nodes, elements = _c(nodes, BVHNODE), _c(elements, np.uint32)
        _check(lib().rt_scene_set_mesh(self._h, int(index), _p(v), len(v), _p(f), len(f), _p(vn), len(vn),
                                       _p(fn), _p(nodes), len(nodes), _p(elements)))
        if vt is not None and len(vt):
            self.set_mesh_texcoords(index, vt, ft)

    def update_mesh_vertices(self, index, v, vn=None, rebuild=False, max_ratio=None, keep_previous=False):
        """new positions (and normals, unless vn is None) for a mesh whose faces stay: refitted in place on the devices that hold
        the scene; rebuild=True takes set_mesh's path instead (the tree is built again at the next use).  max_ratio (>= 1): the
        refitted tree is measured as well (rt_scene_update_mesh_vertices_auto) and built again at the next use when its SAH cost
        has grown beyond max_ratio times the built tree's; the call then returns mesh_quality()'s dict, else None.
        keep_previous=True (RT_MESH_UPDATE_KEEP_PREVIOUS; goes with either): the positions the mesh had become its previous
        positions, which motion() follows its pixels through; an update without it makes the mesh rigid again.
        rebuild="device" (rt_mi355x.h, "device tree build"): the tree is built again on every device that holds the scene, by the
        device; the call returns the build-info dict.  With max_ratio the device build takes the place of the rebuild at the next
        use, and the quality dict has a "build" entry when it happened."""
        device_build = isinstance(rebuild, str)
        if device_build and rebuild != "device":
            raise ValueError(f"update_mesh_vertices: rebuild is {rebuild!r} (False, True or 'device')")
        if max_ratio is not None and rebuild and not device_build:
            raise ValueError("update_mesh_vertices: rebuild=True and max_ratio exclude each other")
        v = _c(v, np.float32).reshape(-1, 3)
        vn = _c(vn, np.float32).reshape(-1, 3) if vn is not None else None
        mesh = (self._h, int(index), _p(v), len(v), _p(vn), len(vn) if vn is not None else 0)
        keep = MESH_UPDATE_KEEP_PREVIOUS if keep_previous else 0
        if device_build:
            b = MeshBuildInfo(struct_size=C.sizeof(MeshBuildInfo))
            if max_ratio is None:
                _check(lib().rt_scene_update_mesh_vertices_build(*mesh, keep, C.byref(b)))
                return b.as_dict()
            q = MeshQuality(struct_size=C.sizeof(MeshQuality))
            _check(lib().rt_scene_update_mesh_vertices_auto_build(*mesh, max_ratio, keep, C.byref(q), C.byref(b)))
            out = q.as_dict()
            if b.flags:
                out["build"] = b.as_dict()
            return out
        if max_ratio is not None:
            q = MeshQuality(struct_size=C.sizeof(MeshQuality))
            _check(lib().rt_scene_update_mesh_vertices_auto_flags(*mesh, max_ratio, keep, C.byref(q)))
            return q.as_dict()
        _check(lib().rt_scene_update_mesh_vertices_flags(*mesh, (MESH_UPDATE_REBUILD if rebuild else 0) | keep))

    def set_mesh_skin(self, index, bone_index, weight, n_bones=None):
        """binds a skin to mesh `index` (rt_mi355x.h, "mesh skinning"): four influences a vertex -- bone_index uint16 (nv, 4), weight
        float32 (nv, 4), used as given -- with the positions the mesh holds now as the rest pose.  n_bones: None = the largest
        index + 1."""
        idx, w = _c(bone_index, np.uint16).reshape(-1, 4), _c(weight, np.float32).reshape(-1, 4)
        if len(idx) != len(w):
            raise ValueError(f"set_mesh_skin: {len(idx)} index rows, {len(w)} weight rows")
        n = int(idx.max()) + 1 if n_bones is None else int(n_bones)
        _check(lib().rt_scene_set_mesh_skin(self._h, int(index), n, _p(idx), _p(w), len(idx)))

    def clear_mesh_skin(self, index):
        """unbinds the skin of mesh `index`; the mesh keeps the positions it has"""
        _check(lib().rt_scene_clear_mesh_skin(self._h, int(index)))

    def mesh_skin(self, index):
        """dict(bound, n_bones, nv, store_current): the skin of mesh `index`, and whether the store's positions are the last pose's
        (0 while the host mirror still owes them: it runs when they are next read)"""
        info = MeshSkinInfo(struct_size=C.sizeof(MeshSkinInfo))
        _check(lib().rt_scene_mesh_skin_info(self._h, int(index), C.byref(info)))
        return dict(bound=bool(info.bound), n_bones=info.n_bones, nv=info.nv, store_current=int(info.store_current))

    def set_mesh_morphs(self, index, deltas):
        """binds a morph set to mesh `index` (rt_mi355x.h, "morph targets"): deltas float32 (n_targets, nv, 3), dense, with the
        positions the mesh holds now as the base"""
        d = _c(deltas, np.float32)
        if d.ndim != 3 or d.shape[2] != 3:
            raise ValueError(f"set_mesh_morphs: deltas has shape {d.shape} ((n_targets, nv, 3))")
        _check(lib().rt_scene_set_mesh_morphs(self._h, int(index), d.shape[0], _p(d), d.shape[1]))

    def clear_mesh_morphs(self, index):
        """unbinds the morph set of mesh `index`; the mesh keeps the positions it has"""
        _check(lib().rt_scene_clear_mesh_morphs(self._h, int(index)))

    def mesh_morphs(self, index):
        """dict(bound, n_targets, nv, store_current): the morph set of mesh `index`, and whether the store's positions are the last
        pose's (0 while the host mirrors still owe them: they run when the positions are next read)"""
        info = MeshMorphInfo(struct_size=C.sizeof(MeshMorphInfo))
        _check(lib().rt_scene_mesh_morph_info(self._h, int(index), C.byref(info)))
        return dict(bound=bool(info.bound), n_targets=info.n_targets, nv=info.nv, store_current=int(info.store_current))

    def mesh_morph_ms(self, device=0):
        """milliseconds of the last k_mesh_pose launch for a morph pose on `device`, by HIP events (RtError RT_ERR_STATE when it ran none)"""
        ms = C.c_float()
        _check(lib().rt_scene_mesh_morph_ms(self._h, device, C.byref(ms)))
        return ms.value

    def pose_mesh(self, index, bones=None, keep_previous=False, rebuild=False, max_ratio=None, morph_weights=None):
        """poses the skinned mesh `index`: bones is float32 (n_bones, 3, 4), row-major, in the mesh's object space.  Everything else
        is update_mesh_vertices(v=the posed positions, vn=None, ...) -- the same arguments, the same return values -- but the
        positions are computed by k_mesh_pose on the devices that hold the scene, from 48 bytes a bone.
        morph_weights (float32 (n_targets,), one a target of the set set_mesh_morphs bound): the morph targets are applied first, and
        bones, which may then be None, to the morphed positions -- the same kernel, from 8 bytes a non-zero weight."""
        if morph_weights is not None:
            return self._morph_mesh(index, morph_weights, bones, keep_previous, rebuild, max_ratio)
        if bones is None:
            raise ValueError("pose_mesh: bones is required without morph_weights")
        device_build = isinstance(rebuild, str)
        if device_build and rebuild != "device":
            raise ValueError(f"pose_mesh: rebuild is {rebuild!r} (False, True or 'device')")
        if max_ratio is not None and rebuild and not device_build:
            raise ValueError("pose_mesh: rebuild=True and max_ratio exclude each other")
        bones = _c(bones, np.float32).reshape(-1, 3, 4)
        pose = (self._h, int(index), _p(bones), len(bones))
        keep = MESH_UPDATE_KEEP_PREVIOUS if keep_previous else 0
        if device_build:
            b = MeshBuildInfo(struct_size=C.sizeof(MeshBuildInfo))
            if max_ratio is None:
                _check(lib().rt_scene_pose_mesh_build(*pose, keep, C.byref(b)))
                return b.as_dict()
            q = MeshQuality(struct_size=C.sizeof(MeshQuality))
            _check(lib().rt_scene_pose_mesh_auto_build(*pose, keep, max_ratio, C.byref(q), C.byref(b)))
            out = q.as_dict()
            if b.flags:
                out["build"] = b.as_dict()
            return out
        if max_ratio is not None:
            q = MeshQuality(struct_size=C.sizeof(MeshQuality))
            _check(lib().rt_scene_pose_mesh_auto(*pose, keep, max_ratio, C.byref(q)))
            return q.as_dict()
        _check(lib().rt_scene_pose_mesh(*pose, (MESH_UPDATE_REBUILD if rebuild else 0) | keep))

    def _morph_mesh(self, index, weights, bones, keep_previous, rebuild, max_ratio):
        """pose_mesh with morph_weights: the rt_scene_morph_mesh* forms"""
        device_build = isinstance(rebuild, str)
        if device_build and rebuild != "device":
            raise ValueError(f"pose_mesh: rebuild is {rebuild!r} (False, True or 'device')")
        if max_ratio is not None and rebuild and not device_build:
            raise ValueError("pose_mesh: rebuild=True and max_ratio exclude each other")
        w = _c(weights, np.float32).reshape(-1)
        bones = None if bones is None else _c(bones, np.float32).reshape(-1, 3, 4)
        pose = (self._h, int(index), _p(w), len(w), _p(bones), 0 if bones is None else len(bones))
        keep = MESH_UPDATE_KEEP_PREVIOUS if keep_previous else 0
        if device_build:
            b = MeshBuildInfo(struct_size=C.sizeof(MeshBuildInfo))
            if max_ratio is None:
                _check(lib().rt_scene_morph_mesh_build(*pose, keep, C.byref(b)))
                return b.as_dict()
            q = MeshQuality(struct_size=C.sizeof(MeshQuality))
            _check(lib().rt_scene_morph_mesh_auto_build(*pose, keep, max_ratio, C.byref(q), C.byref(b)))
            out = q.as_dict()
            if b.flags:
                out["build"] = b.as_dict()
            return out
        if max_ratio is not None:
            q = MeshQuality(struct_size=C.sizeof(MeshQuality))
            _check(lib().rt_scene_morph_mesh_auto(*pose, keep, max_ratio, C.byref(q)))
            return q.as_dict()
        _check(lib().rt_scene_morph_mesh(*pose, (MESH_UPDATE_REBUILD if rebuild else 0) | keep))

    def mesh_skin_ms(self, device=0):
        """milliseconds of the last k_mesh_pose launch for a bone pose on `device`, by HIP events (RtError RT_ERR_STATE when it ran none)"""
        ms = C.c_float()
        _check(lib().rt_scene_mesh_skin_ms(self._h, device, C.byref(ms)))
        return ms.value

    def set_mesh_normals(self, index, mode):
        """what an update without normals leaves mesh `index` with: "stored" (the default: the normals it had) or "smooth" -- its
        smooth normals computed again for the new positions, on the devices that hold the scene (rt_mi355x.h, "smooth normals")"""
        modes = {"stored": MESH_NORMALS_STORED, "smooth": MESH_NORMALS_SMOOTH}
        if mode not in modes:
            raise ValueError(f"set_mesh_normals: mode is {mode!r} ('stored' or 'smooth')")
        _check(lib().rt_scene_set_mesh_normals_mode(self._h, int(index), modes[mode]))

    def mesh_normals(self, index):
        """the mode of mesh `index`: "stored" or "smooth" """
        mode = C.c_uint32()
        _check(lib().rt_scene_get_mesh_normals_mode(self._h, int(index), C.byref(mode)))
        return {MESH_NORMALS_STORED: "stored", MESH_NORMALS_SMOOTH: "smooth"}[mode.value]

    def mesh_normals_ms(self, device=0):
        """milliseconds of the last k_mesh_normals launch on `device`, by HIP events (RtError RT_ERR_STATE when it ran none)"""
        ms = C.c_float()
        _check(lib().rt_scene_mesh_normals_ms(self._h, device, C.byref(ms)))
        return ms.value

    def previous_positions(self):
        """how many meshes of the scene hold previous positions (from the scene store: no GPU)"""
        n = C.c_int32()
        _check(lib().rt_scene_previous_positions(self._h, C.byref(n)))
        return n.value

    def mesh_device_previous(self, index, device=0):
        """the previous positions of mesh `index` as they sit on `device` (lowered there first if need be): float32 (nv, 3), or
        None when the mesh holds none"""
        n = C.c_uint32()
        _check(lib().rt_scene_mesh_device_previous(self._h, device, int(index), None, 0, C.byref(n)))
        if n.value == 0:
            return None
        out = np.zeros((n.value, 3), np.float32)
        _check(lib().rt_scene_mesh_device_previous(self._h, device, int(index), _p(out), len(out), C.byref(n)))
        return out

    def motion(self, cam, prev_cam, prev_nodes, z, object_id, depth_tol=0.05, device=0, shade_model=SHADE_FIN):
        """rt_scene_motion on host arrays: capi.motion() with the scene's own nodes as this frame's, and the pixels of every mesh
        that holds previous positions (update_mesh_vertices(keep_previous=True)) followed through the deformation (rt_mi355x.h,
        "motion vectors for deforming meshes").  shade_model: the model the frame was rendered with (whose triangle test walks the
        meshes: SHADE_FIN's two-sided one, or the back-face-culled one of every other model).  prev_nodes: the NODE array of the previous frame (None: the nodes did not move).
        Returns float32 (H, W, 3): fx, fy, z_exp (z_exp <= 0: no previous position)."""
        prev = _c(prev_nodes, NODE) if prev_nodes is not None else None
        z, ids = _c(z, np.float32), _c(object_id, np.int32)
        h, w = cam.height, cam.width
        assert z.shape == ids.shape == (h, w)
        out = np.empty((h, w, 3), np.float32)
        pl = MotionPlanes(z=z.ctypes.data, object_id=ids.ctypes.data, motion=out.ctypes.data)
        _check(lib().rt_scene_motion(self._h, int(shade_model), device, C.byref(cam), C.byref(prev_cam), _p(prev),
                                     len(prev) if prev is not None else self.counts()["nodes"], depth_tol, C.byref(pl)))
        return out

    def motion_device(self, device, stream, cam, prev_cam, prev_nodes, *, z_ptr, object_id_ptr, motion_ptr, depth_tol=0.05, sync=True,
                      shade_model=SHADE_FIN):
        """rt_scene_motion_device: the same on image-sized DEVICE planes, enqueued on `stream` (an explicit stream's handle; None =
        the null stream of the device).  prev_nodes stays a host array; it is consumed before the call returns."""
        prev = _c(prev_nodes, NODE) if prev_nodes is not None else None
        pl = MotionPlanes(z=z_ptr, object_id=object_id_ptr, motion=motion_ptr)
        _check(lib().rt_scene_motion_device(self._h, int(shade_model), device, _stream_handle(stream), C.byref(cam), C.byref(prev_cam),
                                            _p(prev), len(prev) if prev is not None else self.counts()["nodes"],
                                            depth_tol, C.byref(pl), 1 if sync else 0))

    def mesh_quality(self, index, device=0):
        """the SAH cost of mesh `index`'s tree as it sits on `device` (lowered there first if need be), by k_bvh_cost:
        dict(cost, built_cost, ratio, measure_ms, degenerate, rebuilt, not_on_device)"""
        q = MeshQuality(struct_size=C.sizeof(MeshQuality))
        _check(lib().rt_scene_mesh_quality(self._h, device, int(index), C.byref(q)))
        return q.as_dict()

    def mesh_update_ms(self, device=0):
        """the last in-place update on `device`: dict(upload, retri, refit in ms by HIP events, level_launches)"""
        t = MeshUpdateMs(struct_size=C.sizeof(MeshUpdateMs))
        _check(lib().rt_scene_mesh_update_ms(self._h, device, C.byref(t)))
        return dict(upload=t.upload, retri=t.retri, refit=t.refit, level_launches=t.level_launches)

    def set_mesh_texcoords(self, index, vt, ft):
        """cyTriMesh VT/FT of a mesh already set (read by the PROJ13-family triangle)."""
        vt, ft = _c(vt, np.float32).reshape(-1, 3), _c(ft, np.uint32).reshape(-1, 3)
        _check(lib().rt_scene_set_mesh_texcoords(self._h, int(index), _p(vt), len(vt), _p(ft)))

    def set_materials(self, m):
        m = _c(m, BLINN)
        _check(lib().rt_scene_set_materials(self._h, _p(m), len(m)))

    def set_lights(self, l):
        l = _c(l, LIGHT)
        _check(lib().rt_scene_set_lights(self._h, _p(l), len(l)))

    def set_environment(self, env=(0, 0, 0), bg=(0, 0, 0)):
        e, b = (C.c_float * 3)(*env), (C.c_float * 3)(*bg)
        _check(lib().rt_scene_set_environment(self._h, e, b))

    def set_textures(self, textures, texels):
        textures, texels = _c(textures, TEXTURE), _c(texels, np.uint8)
        _check(lib().rt_scene_set_textures(self._h, _p(textures), len(textures), _p(texels), texels.size))

    def set_material_maps(self, maps):
        maps = _c(maps, TEXMAP)
        assert len(maps) % 2 == 0
        _check(lib().rt_scene_set_material_maps(self._h, _p(maps), len(maps) // 2))

    def set_environment_maps(self, environment=None, background=None):
        e = _c(environment, TEXMAP).reshape(1) if environment is not None else None
        b = _c(background, TEXMAP).reshape(1) if background is not None else None
        _check(lib().rt_scene_set_environment_maps(self._h, _p(e), _p(b)))

    def set_photons(self, balanced_1based):
        if balanced_1based is None or len(balanced_1based) < 2:
            _check(lib().rt_scene_set_photons(self._h, None, 0))
            return
        a = _c(balanced_1based, PHOTON)
        _check(lib().rt_scene_set_photons(self._h, _p(a), len(a) - 1))

    def set_caustic_photons(self, balanced_1based):
        """the second map (P13's causticmap): same format as set_photons; used when params.caustic_k > 0"""
        if balanced_1based is None or len(balanced_1based) < 2:
            _check(lib().rt_scene_set_caustic_photons(self._h, None, 0))
            return
        a = _c(balanced_1based, PHOTON)
        _check(lib().rt_scene_set_caustic_photons(self._h, _p(a), len(a) - 1))

    def generate_photons(self, max_photons=1000000, photon_bounce=8, seed=20171203, device=0, dat_path=None):
        """generatePhotonMap as a whole on the GPU (photon pass -> [dump] -> queryable structure); returns the stage times"""
        ms = SetupMs()
        _check(lib().rt_scene_generate_photons(self._h, device, int(max_photons), int(photon_bounce), int(seed),
                                               os.fsencode(dat_path) if dat_path else None, C.byref(ms)))
        return ms

    def set_render_flags(self, flags):
        """RENDER_* bits or 0 (the default); refused while a job on this scene is live"""
        _check(lib().rt_scene_set_render_flags(self._h, int(flags)))

    def render_flags(self):
        f = C.c_uint32()
        _check(lib().rt_scene_get_render_flags(self._h, C.byref(f)))
        return f.value

    def material_classes(self):
        """the class word of every material as the lowering sets it (MAT_* bits; all 0 under RENDER_GENERAL_SHADING): host only"""
        n = C.c_int32()
        _check(lib().rt_scene_material_classes(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint32)
        if n.value:
            _check(lib().rt_scene_material_classes(self._h, _p(out), n.value, None))
        return out

    def set_photon_dump(self, dat_path):
        _check(lib().rt_scene_set_photon_dump(self._h, os.fsencode(dat_path) if dat_path else None))

    def get_photons(self):
        """the scene's photon map in the reference's balanced form (1-based; empty array when there is none)"""
        n = C.c_uint32()
        _check(lib().rt_scene_get_photons(self._h, None, 0, C.byref(n)))
        if n.value == 0:
            return np.zeros(0, PHOTON)
        out = np.zeros(n.value + 1, PHOTON)
        _check(lib().rt_scene_get_photons(self._h, _p(out), len(out), None))
        return out

    def load_xml(self, path):
        _check(lib().rt_scene_load_xml(self._h, os.fsencode(path)))

    # -- getters -------------------------------------------------------------------------------
    def camera(self):
        cam = Camera()
        _check(lib().rt_scene_get_camera(self._h, C.byref(cam)))
        return cam

    def counts(self):
        n = [C.c_int32() for _ in range(4)]
        nph = C.c_uint32()
        _check(lib().rt_scene_counts(self._h, *[C.byref(x) for x in n], C.byref(nph)))
        return dict(nodes=n[0].value, meshes=n[1].value, materials=n[2].value, lights=n[3].value, photons=nph.value)

    def get_nodes(self):
        """the scene's node array (NODE records), as rt_scene_set_nodes took it"""
        nodes = np.zeros(self.counts()["nodes"], NODE)
        _check(lib().rt_scene_get_nodes(self._h, _p(nodes), len(nodes)))
        return nodes

    def export(self):
        """All host-side arrays (for handing the same bytes to another consumer)."""
        c = self.counts()
        nodes = np.zeros(c["nodes"], NODE)
        mats = np.zeros(c["materials"], BLINN)
        lights = np.zeros(c["lights"], LIGHT)
        _check(lib().rt_scene_get_nodes(self._h, _p(nodes), len(nodes)))
        if len(mats):
            _check(lib().rt_scene_get_materials(self._h, _p(mats), len(mats)))
        if len(lights):
            _check(lib().rt_scene_get_lights(self._h, _p(lights), len(lights)))
        meshes = []
        for m in range(c["meshes"]):
            k = [C.c_int32() for _ in range(4)]
            _check(lib().rt_scene_mesh_counts(self._h, m, *[C.byref(x) for x in k]))
            nv, nf, nvn, nn = (x.value for x in k)
            d = dict(v=np.zeros((nv, 3), np.float32), f=np.zeros((nf, 3), np.uint32),
                     vn=np.zeros((nvn, 3), np.float32), fn=np.zeros((nf, 3), np.uint32),
                     nodes=np.zeros(nn, BVHNODE), elements=np.zeros(nf, np.uint32))
            _check(lib().rt_scene_get_mesh(self._h, m, _p(d["v"]), _p(d["f"]), _p(d["vn"]), _p(d["fn"]),
                                           _p(d["nodes"]), _p(d["elements"])))
            nvt = C.c_int32()
            _check(lib().rt_scene_get_mesh_texcoords(self._h, m, C.byref(nvt), None, None))
            d["vt"], d["ft"] = np.zeros((nvt.value, 3), np.float32), np.zeros((nf if nvt.value else 0, 3), np.uint32)
            if nvt.value:
                _check(lib().rt_scene_get_mesh_texcoords(self._h, m, None, _p(d["vt"]), _p(d["ft"])))
            meshes.append(d)
        ntex, nbytes = C.c_int32(), C.c_uint64()
        _check(lib().rt_scene_get_textures(self._h, None, 0, None, 0, C.byref(ntex), C.byref(nbytes)))
        textures, texels = np.zeros(ntex.value, TEXTURE), np.zeros(nbytes.value, np.uint8)
        _check(lib().rt_scene_get_textures(self._h, _p(textures), len(textures), _p(texels), texels.size, None, None))
        maps, env_map, bg_map = np.zeros(2 * len(mats), TEXMAP), np.zeros(1, TEXMAP), np.zeros(1, TEXMAP)
        _check(lib().rt_scene_get_maps(self._h, _p(maps), len(maps), _p(env_map), _p(bg_map)))
        has_maps = bool(len(maps)) and bool((maps["tm"] != 0).any() or (maps["texture"] != 0).any())
        env, bg = np.zeros(3, np.float32), np.zeros(3, np.float32)
        _check(lib().rt_scene_get_environment(self._h, _p(env), _p(bg)))
        return dict(nodes=nodes, materials=mats, lights=lights, meshes=meshes, textures=textures, texels=texels,
                    material_maps=maps if has_maps else None, env_map=env_map, bg_map=bg_map, env=env, bg=bg)

    def mesh_device_bvh(self, index):
        """the tree the kernels walk for mesh `index`, built on the host (no GPU): (DEVBVHNODE records, face of every triangle
        slot, DeviceBvhInfo with root_ref, stack_need and the compiled stack sizes)"""
        info = DeviceBvhInfo(struct_size=C.sizeof(DeviceBvhInfo))
        _check(lib().rt_scene_mesh_device_bvh(self._h, int(index), C.byref(info), None, 0, None, 0))
        nodes, slot_face = np.zeros(info.n_nodes, DEVBVHNODE), np.zeros(info.n_slots, np.uint32)
        _check(lib().rt_scene_mesh_device_bvh(self._h, int(index), C.byref(info), _p(nodes), len(nodes), _p(slot_face), len(slot_face)))
        return nodes, slot_face, info

    def mesh_device_read(self, index, device=0):
        """what sits on `device` for mesh `index` right now (the scene is lowered there first if need be): dict(info, nodes,
        slot_face, tris [slots, 12]: A B C N, nrm [slots, 9], root_box [6])"""
        info = DeviceBvhInfo(struct_size=C.sizeof(DeviceBvhInfo))
        _check(lib().rt_scene_mesh_device_read(self._h, device, int(index), C.byref(info), None, 0, None, 0, None, None, None))
        n = info.n_slots
        out = dict(info=info, nodes=np.zeros(info.n_nodes, DEVBVHNODE), slot_face=np.zeros(n, np.uint32),
                   tris=np.zeros((n, 12), np.float32), nrm=np.zeros((n, 9), np.float32), root_box=np.zeros(6, np.float32))
        _check(lib().rt_scene_mesh_device_read(self._h, device, int(index), C.byref(info), _p(out["nodes"]), len(out["nodes"]),
                                               _p(out["slot_face"]), n, _p(out["tris"]), _p(out["nrm"]), _p(out["root_box"])))
        return out

    # -- GPU work -------------------------------------------------------------------------------
    def trace_rays(self, rays, shade_model=SHADE_FIN, device=0):
        rays = _c(rays, np.float32).reshape(-1, 6)
        n = len(rays)
        out = dict(hit=np.zeros(n, np.uint8), z=np.zeros(n, np.float32), p=np.zeros((n, 3), np.float32),
                   N=np.zeros((n, 3), np.float32), node=np.zeros(n, np.int32), front=np.zeros(n, np.uint8))
        _check(lib().rt_trace_rays(self._h, int(shade_model), device, _p(rays), n, _p(out["hit"]),
                                   _p(out["z"]), _p(out["p"]), _p(out["N"]), _p(out["node"]), _p(out["front"])))
        return out

    def estimate_irradiance(self, k, radius, pos, normal, device=0):
        pos, normal = _c(pos, np.float32).reshape(-1, 3), _c(normal, np.float32).reshape(-1, 3)
        irr, d = np.zeros_like(pos), np.zeros_like(pos)
        _check(lib().rt_estimate_irradiance(self._h, device, int(k), radius, _p(pos), _p(normal), len(pos), _p(irr), _p(d)))
        return irr, d

    def shade_rays(self, params, rays, device=0):
        rays = _c(rays, np.float32).reshape(-1, 6)
        n = len(rays)
        hit, rgb, z = np.zeros(n, np.uint8), np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
        _check(lib().rt_shade_rays(self._h, C.byref(params), device, _p(rays), n, _p(hit), _p(rgb), _p(z)))
        return hit, rgb, z

    def photon_pass(self, max_photons, photon_bounce=8, seed=20171203, device=0):
        """generatePhotonMap on the GPU: returns (unbalanced 1-based photon array, attempts)."""
        out = np.zeros(int(max_photons) + 9, PHOTON)
        n, att = C.c_uint32(), C.c_uint64()
        _check(lib().rt_photon_pass(self._h, device, int(max_photons), int(photon_bounce), int(seed), _p(out), len(out),
                                    C.byref(n), C.byref(att)))
        return out[: n.value + 1].copy(), att.value

    def caustic_pass(self, max_diffuse_hits, photon_bounce=5, seed=20171203, device=0):
        """P13's caustic loop on the GPU: returns (unbalanced 1-based photon array, attempts)."""
        out = np.zeros(int(max_diffuse_hits) + 9, PHOTON)
        n, att = C.c_uint32(), C.c_uint64()
        _check(lib().rt_caustic_pass(self._h, device, int(max_diffuse_hits), int(photon_bounce), int(seed), _p(out), len(out),
                                     C.byref(n), C.byref(att)))
        return out[: n.value + 1].copy(), att.value

    def render(self, cam, params, tiles=None, device=0, photon_pass=False):
        """Blocking render through the asynchronous job API (rt_render_begin + rt_render_wait).  photon_pass=False (the
        tests' default) renders the scene's photon map as it is: params.photon_count is taken as 0 for this call;
        photon_pass=True leaves it alone, so that rt_render_begin first runs generatePhotonMap like BeginRender does."""
        return self._render(cam, params, tiles, device, photon_pass, None)

    def render_linear(self, cam, params, tiles=None, device=0, photon_pass=False, fill=0.0):
        """render() plus the linear (pre-gamma) float RGB plane, through rt_render_begin_linear:
        (rgb, z, cnt, linear (H, W, 3) float32, stats, progress).  Pixels outside `tiles` keep `fill`."""
        linear = np.full((cam.height, cam.width, 3), fill, np.float32)
        rgb, z, cnt, st, progress = self._render(cam, params, tiles, device, photon_pass, linear)
        return rgb, z, cnt, linear, st, progress

    def render_outputs(self, cam, params, planes=FEATURE_PLANES, tiles=None, device=0, photon_pass=False, fill=0.0, id_fill=-1):
        """render() with the optional planes named in `planes` (any of linear, normal, albedo, alpha, object_id, variance),
        through rt_render_begin_outputs (with "variance": rt_render_begin_outputs_var): a dict with rgb, z, count, stats,
        progress and one array per plane asked for -- float32 (H, W, 3) for linear / normal / albedo / variance, float32 (H, W)
        for alpha, int32 (H, W) for object_id.  Pixels outside `tiles` keep `fill` (object_id: `id_fill`)."""
        h, w = cam.height, cam.width
        out = {}
        for name in planes:
            _, dtype, ch = OUTPUT_PLANES[name]          # KeyError: no such plane
            out[name] = np.full((h, w, 3) if ch == 3 else (h, w), id_fill if name == "object_id" else fill, dtype)
        out["rgb"], out["z"], out["count"], out["stats"], out["progress"] = self._render(cam, params, tiles, device, photon_pass, None, dict(out))
        return out

    def render_denoised(self, cam, params, device=0, photon_pass=False, variance=False, exposure=None, tonemap_kw=None, bloom=None,
                        bloom_kw=None, depth_of_field=None, dof_kw=None, **denoise_kw):
        """render_outputs with the linear plane and the four feature planes, then denoise() of that frame guided by them
        (gamma: the render's): the same dict with "denoised" (float32 (H, W, 3), linear) and "denoised_rgb" (uint8 (H, W, 3))
        added.  denoise_kw: levels, sigma_color, sigma_normal, sigma_depth.  variance=True: the render also fills
        out["variance"] and the denoise is the variance-guided one (denoise_kw: also k_sigma); "denoised_variance" is added.
        exposure: an Exposure on `device` -- the denoised plane is metered (with the frame's object_id) and tone-mapped, and
        "display_rgb" (uint8 (H, W, 3)) is added; tonemap_kw: a dict of Exposure.tonemap's keywords (operator, key, ...).
        bloom: a Bloom of the camera's size on `device` -- the denoised plane is bloomed first (relative to the scale `exposure`
        holds from the frame before; bloom_kw: a dict of Bloom.apply's keywords), "bloomed" (float32 (H, W, 3)) is added and
        "display_rgb" is made from it.
        depth_of_field: a DepthOfField of the camera's size on `device` -- the frame is rendered PINHOLE (a copy of `cam` with
        dof = 0: exact planes) and the denoised plane is defocused from "z" with cam's own dof (dof_kw: a dict of
        DepthOfField.apply's keywords); "defocused" (float32 (H, W, 3)) and "coc" (float32 (H, W), the signed circle of confusion
        in pixels) are added, and bloom and tone mapping run on the defocused plane."""
        planes = ("linear",) + FEATURE_PLANES + (("variance",) if variance else ())
        out = self.render_outputs(_pinhole(cam) if depth_of_field is not None else cam, params, planes=planes, device=device, photon_pass=photon_pass)
        denoise_kw.setdefault("gamma", params.gamma)
        if variance:
            out["denoised"], out["denoised_rgb"], out["denoised_variance"] = denoise(
                out["linear"], out["normal"], out["albedo"], out["z"], out["object_id"], rgb8=True, device=device,
                variance=out["variance"], return_variance=True, **denoise_kw)
        else:
            out["denoised"], out["denoised_rgb"] = denoise(out["linear"], out["normal"], out["albedo"], out["z"], out["object_id"],
                                                           rgb8=True, device=device, **denoise_kw)
        return self._finish_frame(out, out["denoised"], params, None, None, bloom, bloom_kw, exposure, tonemap_kw, depth_of_field, dof_kw, cam)

    def render_temporal(self, history, cam, params, device=0, denoise=True, exposure=None, tonemap_kw=None, moving=False, clip=None,
                        bloom=None, bloom_kw=None, motion_blur=None, motion_blur_kw=None, depth_of_field=None, dof_kw=None, **kw):
        """One frame of a stream of frames: render_outputs with the linear, feature and variance planes, then
        history.accumulate() of that frame (a History of the camera's size on `device`): the same dict with "accumulated" and
        "accumulated_variance" (float32 (H, W, 3)) and "history" (float32 (H, W), the per-pixel history length) added.
        denoise=True: then the variance-guided denoise() of the accumulated pair, "denoised" and "denoised_rgb" added.
        kw: photon_pass; alpha, max_history (the accumulation); levels, sigma_color, k_sigma (the denoise); sigma_normal,
        sigma_depth (both).  gamma is the render's.
        exposure: an Exposure on `device` -- the final linear plane (the denoised one, or the accumulated one when
        denoise=False) is metered with the frame's object_id and tone-mapped, "display_rgb" (uint8 (H, W, 3)) added; tonemap_kw:
        a dict of Exposure.tonemap's keywords (operator, key, adapt_up, ...).
        moving=True: nodes may have moved since the previous frame (set_nodes).  `history` remembers the camera and the node
        array of the frame it last accumulated through this method; the motion plane from there to this frame is computed on
        the device (motion()) from the scene's current nodes and the accumulation takes its reprojection from it;
        "motion" (float32 (H, W, 3)) is added.  The first frame (and the first after history.reset()) has nothing to compare
        with: prev_nodes=None and prev_cam = cam.  A frame that reaches `history` any other way -- render_temporal without
        moving=True, accumulate(), accumulate_device() -- makes it forget the remembered frame: the next moving=True frame then
        takes the nodes as not moved since, and the camera from the history as rt_temporal does (prev_cam cannot be known here,
        so that frame is accumulated WITHOUT a motion plane; "motion" is still added, computed with prev_cam = cam).
        When a mesh of the scene holds previous positions (update_mesh_vertices(keep_previous=True)) the plane is the scene's
        own (Scene.motion, with params.shade_model), which follows the deformed surface; for every other
        scene it is capi.motion's, as it always was.
        clip: history rectification, as History.accumulate's (True, or a dict of radius, k_clip, min_count, clip_history);
        "clipped" (float32 (H, W): 0 no history, 1 kept, 2 clipped) is added.  Works with moving=True.
        bloom: a Bloom of the camera's size on `device` -- the final linear plane is bloomed before it is tone-mapped, as in
        render_denoised: "bloomed" is added and "display_rgb" is made from it; bloom_kw: a dict of Bloom.apply's keywords.
        motion_blur: a MotionBlur of the camera's size on `device`; needs moving=True (ValueError without it) -- the final linear
        plane is blurred along the frame's "motion" plane with its "z" (motion_blur_kw: a dict of MotionBlur.apply's keywords),
        "motion_blurred" (float32 (H, W, 3)) is added, and bloom and tone mapping run on it.
        depth_of_field: a DepthOfField of the camera's size on `device`, as in render_denoised: the frame is rendered pinhole, so
        the planes, the reprojection and the motion vectors are exact, and the final linear plane is defocused with cam's own
        dof ahead of the motion blur; "defocused" and "coc" are added (dof_kw: a dict of DepthOfField.apply's keywords)."""
        if motion_blur is not None and not moving:
            raise ValueError("render_temporal: motion_blur needs moving=True (the frame's motion plane)")
        photon_pass = kw.pop("photon_pass", False)
        t_kw = {k: kw[k] for k in ("alpha", "max_history", "sigma_normal", "sigma_depth") if k in kw}
        d_kw = {k: kw[k] for k in ("levels", "sigma_color", "k_sigma", "sigma_normal", "sigma_depth") if k in kw}
        unknown = set(kw) - set(t_kw) - set(d_kw)
        if unknown:
            raise TypeError(f"no render_temporal parameter {sorted(unknown)[0]!r}")
        out = self.render_outputs(_pinhole(cam) if depth_of_field is not None else cam, params, planes=("linear",) + FEATURE_PLANES + ("variance",),
                                  device=device, photon_pass=photon_pass)
        if moving:
            out["motion"], known, remember = self._motion_since(history, cam, out["z"], out["object_id"], device, params.shade_model)
            if known:
                t_kw["motion"] = out["motion"]
        if clip is not None:
            t_kw.update(clip=clip, return_clipped=True)
        res = history.accumulate(cam, out["linear"], out["normal"], out["albedo"], out["z"], out["object_id"], variance=out["variance"],
                                 return_history=True, gamma=params.gamma, **t_kw)
        out["accumulated"], out["accumulated_variance"], out["history"] = res[:3]
        if clip is not None:
            out["clipped"] = res[3]
        if moving:
            history._moving = remember                  # (accumulate() forgot it: only this method knows the frame's nodes)
        if denoise:
            out["denoised"], out["denoised_rgb"] = _denoise(
                out["accumulated"], out["normal"], out["albedo"], out["z"], out["object_id"], rgb8=True, device=device,
                variance=out["accumulated_variance"], gamma=params.gamma, **d_kw)
        return self._finish_frame(out, out["denoised" if denoise else "accumulated"], params, motion_blur, motion_blur_kw, bloom, bloom_kw,
                                  exposure, tonemap_kw, depth_of_field, dof_kw, cam)

    @staticmethod
    def _finish_frame(out, final, params, motion_blur, motion_blur_kw, bloom, bloom_kw, exposure, tonemap_kw, depth_of_field=None, dof_kw=None,
                      cam=None):
        """the tail of render_denoised and render_temporal on the frame's final linear plane: depth of field (with `cam`, the
        caller's camera and its dof), then motion blur, then bloom, then tone mapping, each only where its object is given; adds
        "defocused" and "coc", "motion_blurred", "bloomed" and "display_rgb" to `out`"""
        if depth_of_field is not None:
            final, out["coc"] = depth_of_field.apply(final, out["z"], cam, return_coc=True, **(dof_kw or {}))
            out["defocused"] = final
        if motion_blur is not None:
            final = out["motion_blurred"] = motion_blur.apply(final, out["motion"], out["z"], **(motion_blur_kw or {}))
        if bloom is not None:
            final = out["bloomed"] = bloom.apply(final, exposure=exposure, **(bloom_kw or {}))
        if exposure is not None:
            out["display_rgb"] = exposure.tonemap(final, out["object_id"], **dict({"gamma": params.gamma}, **(tonemap_kw or {})))
        return out

    def _motion_since(self, history, cam, z, object_id, device, shade_model=SHADE_FIN):
        """render_temporal(moving=True): (the motion plane from the frame `history` remembers to this one, computed on the
        device; whether the frame the history holds is the remembered one, so that the plane may replace the reprojection; what
        to remember of this frame)"""
        nodes = self.get_nodes()
        first = history.frames == 0
        known = first or (history._moving is not None and len(history._moving[1]) == len(nodes))
        prev_cam, prev_nodes = history._moving if known and not first else (cam, None)
        if self.previous_positions():            # a mesh was deformed with keep_previous: the scene form, which follows its pixels
            plane = self.motion(cam, prev_cam, prev_nodes, z, object_id, device=device, shade_model=shade_model)
        else:
            plane = motion(cam, prev_cam, nodes, prev_nodes, z, object_id, device=device)
        return plane, known, (_copy_camera(cam), nodes)

    def _render(self, cam, params, tiles, device, photon_pass, linear, planes=None):
        if not photon_pass and params.photon_count != 0:
            q = Params()
            C.memmove(C.byref(q), C.byref(params), C.sizeof(Params))
            q.photon_count = 0
            params = q
        w, h = cam.width, cam.height
        rgb, z, cnt = np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.float32), np.zeros((h, w), np.uint8)
        tiles = tiles or TileRange(32, 8, 0, 1)
        job = C.c_void_p()
        head = (self._h, C.byref(cam), C.byref(params), C.byref(tiles), device)
        if planes is not None:
            o = Outputs(rgb8=rgb.ctypes.data, z=z.ctypes.data, count=cnt.ctypes.data,
                        **{OUTPUT_PLANES[name][0]: a.ctypes.data for name, a in planes.items() if name != "variance"})
            if "variance" in planes:
                _check(lib().rt_render_begin_outputs_var(*head, C.byref(o), planes["variance"].ctypes.data, C.byref(job)))
            else:
                _check(lib().rt_render_begin_outputs(*head, C.byref(o), C.byref(job)))
        elif linear is None:
            _check(lib().rt_render_begin(*head, _p(rgb), _p(z), _p(cnt), C.byref(job)))
        else:
            _check(lib().rt_render_begin_linear(*head, _p(rgb), _p(z), _p(cnt), _p(linear), C.byref(job)))
        try:
            _check(lib().rt_render_wait(job))
            st = Stats()
            _check(lib().rt_job_stats(job, C.byref(st)))
            progress = lib().rt_render_progress(job)
        finally:
            lib().rt_job_destroy(job)
        return rgb, z, cnt, st, progress

    def _render_tiles(self, entry, cam, params, tiles, device, stream, sync, want_stats, *planes):
        """what the tile-render entry points share: the scene, camera, parameters, tiles, device and stream lead, `planes` (what
        `entry` renders into) follow, sync and the optional rt_stats end the call; returns the Stats"""
        st = Stats()
        _check(getattr(lib(), entry)(self._h, C.byref(cam), C.byref(params), C.byref(tiles), device, _stream_handle(stream), *planes,
                                     1 if sync else 0, C.byref(st) if want_stats else None))
        return st

    def render_tiles_device(self, cam, params, tiles, device, rgb_ptr, z_ptr, cnt_ptr, stream=None, sync=True,
                            want_stats=True, linear_ptr=None):
        """Render this call's tiles into DEVICE buffers (e.g. torch tensors' data_ptr()).
        stream: None = the library's own stream; otherwise the handle of an EXPLICIT hipStream_t.  0 -- what torch
        reports for its legacy default stream -- is refused: through this argument NULL means "the library's
        stream", so work on the default stream would silently not be ordered with the render; run the caller's
        side under a torch.cuda.Stream and pass its handle (raytracing_folder_amd.dist does).
        linear_ptr: also the linear plane (float32 (H, W, 3) on the device), through rt_render_tiles_linear_device."""
        head = (cam, params, tiles, device, stream, sync, want_stats, rgb_ptr, z_ptr, cnt_ptr)
        if linear_ptr is None:
            return self._render_tiles("rt_render_tiles_device", *head)
        return self._render_tiles("rt_render_tiles_linear_device", *head, linear_ptr)

    def render_tiles_outputs_device(self, cam, params, tiles, device, rgb_ptr, z_ptr, cnt_ptr, stream=None, sync=True,
                                    want_stats=True, linear_ptr=None, normal_ptr=None, albedo_ptr=None, alpha_ptr=None,
                                    object_id_ptr=None, variance_ptr=None):
        """render_tiles_device through rt_render_tiles_outputs_device: every *_ptr that is not None names an image-sized
        DEVICE plane to fill (float32 x 3 for linear / normal / albedo, float32 for alpha, int32 for object_id).
        variance_ptr (float32 x 3): through rt_render_tiles_outputs_var_device."""
        o = Outputs(rgb8=rgb_ptr, z=z_ptr, count=cnt_ptr, rgb_linear=linear_ptr, normal=normal_ptr, albedo=albedo_ptr,
                    alpha=alpha_ptr, object_id=object_id_ptr)
        head = (cam, params, tiles, device, stream, sync, want_stats, C.byref(o))
        if variance_ptr is None:
            return self._render_tiles("rt_render_tiles_outputs_device", *head)
        return self._render_tiles("rt_render_tiles_outputs_var_device", *head, variance_ptr)

    def render_tiles_packed_device(self, cam, params, tiles, device, packed_ptr, packed_bytes, stream=None, sync=True,
                                   want_stats=True, linear=False):
        """This call's tiles as packed 8-byte pixel records (the all-gather contribution of a rank), see the header.
        linear=True: 24-byte records that also hold the linear plane (tiles_packed_size(..., linear=True) bytes)."""
        return self._render_tiles("rt_render_tiles_packed_linear_device" if linear else "rt_render_tiles_packed_device", cam, params, tiles,
                                  device, stream, sync, want_stats, packed_ptr, int(packed_bytes))

    def render_tiles_packed_outputs_device(self, cam, params, tiles, device, packed_ptr, packed_bytes, stream=None, sync=True,
                                           want_stats=True, planes=()):
        """render_tiles_packed_device with the planes named in `planes` (those of render_outputs) as sections behind the records:
        one rank's contribution in the packed planes format, tiles_packed_planes_size(..., planes) bytes.  Slots of no pixel are
        zeroed by the call."""
        return self._render_tiles("rt_render_tiles_packed_outputs_device", cam, params, tiles, device, stream, sync, want_stats,
                                  packed_ptr, int(packed_bytes), plane_mask(planes))

    def render_counters(self, device=0, reset=False):
        """the device-side work counters accumulated since they were last cleared (rt_render_counters); waits for pending renders"""
        st = Stats()
        _check(lib().rt_render_counters(self._h, device, 1 if reset else 0, C.byref(st)))
        return st

    def render_check(self, device=0):
        """Collect the verdict of the asynchronous renders issued so far (raises on dropped rays)."""
        _check(lib().rt_render_check(self._h, device))
