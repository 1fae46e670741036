"""The C ABI of librt_mi355x.so (include/rt_mi355x.h) as ctypes sees it: the records, constants and structs, the signature of
every function (SIGNATURES), and the library handle (lib()).  The wrappers are in capi.py and stages.py.

The render entry points run ONLY on the HIP kernels; when the library or a gfx950 device is
missing they raise -- there is no CPU fallback in this package.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "librt_mi355x.so")
CSRC = os.path.join(HERE, "csrc")

# numpy mirrors of the POD records of include/rt_mi355x.h
NODE = np.dtype([("tm", "<f4", 9), ("itm", "<f4", 9), ("pos", "<f4", 3), ("parent", "<i4"),
                 ("obj_type", "<i4"), ("mesh", "<i4"), ("material", "<i4")])
BVHNODE = np.dtype([("box", "<f4", 6), ("data", "<u4")])
BLINN = np.dtype([("diffuse", "<f4", 3), ("specular", "<f4", 3), ("reflection", "<f4", 3),
                  ("refraction", "<f4", 3), ("emission", "<f4", 3), ("absorption", "<f4", 3),
                  ("glossiness", "<f4"), ("ior", "<f4"), ("reflection_glossiness", "<f4"),
                  ("refraction_glossiness", "<f4")])
LIGHT = np.dtype([("type", "<i4"), ("intensity", "<f4", 3), ("position", "<f4", 3),
                  ("direction", "<f4", 3), ("size", "<f4")])
PHOTON = np.dtype([("position", "<f4", 3), ("power", "<f4"), ("color", "u1", 3),
                   ("plane_and_dirz", "u1"), ("dir_x", "<i2"), ("dir_y", "<i2")])
TEXTURE = np.dtype([("type", "<i4"), ("width", "<i4"), ("height", "<i4"), ("texel_offset", "<u4"),
                    ("color1", "<f4", 3), ("color2", "<f4", 3)])
TEXMAP = np.dtype([("texture", "<i4"), ("tm", "<f4", 9), ("itm", "<f4", 9), ("pos", "<f4", 3)])
assert (NODE.itemsize, BVHNODE.itemsize, BLINN.itemsize, LIGHT.itemsize, PHOTON.itemsize,
        TEXTURE.itemsize, TEXMAP.itemsize) == (100, 28, 88, 44, 24, 40, 88)
TEX_FILE, TEX_CHECKER, MAP_NONE, MAP_EMPTY = 1, 2, -1, -2

OBJ_NONE, OBJ_SPHERE, OBJ_PLANE, OBJ_MESH = 0, 1, 2, 3
LIGHT_AMBIENT, LIGHT_DIRECT, LIGHT_POINT = 0, 1, 2
SHADE_FIN, SHADE_P13, SHADE_P12, SHADE_P6, SHADE_P3 = 0, 1, 2, 3, 4


class Camera(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("dir", C.c_float * 3), ("up", C.c_float * 3),
                ("fov", C.c_float), ("focaldist", C.c_float), ("dof", C.c_float),
                ("width", C.c_int32), ("height", C.c_int32)]


class Params(C.Structure):
    _fields_ = [("min_sample", C.c_int32), ("max_sample", C.c_int32), ("threshold", C.c_float),
                ("bounce", C.c_int32), ("hemisphere_sample", C.c_int32), ("knn_k", C.c_int32),
                ("knn_radius", C.c_float), ("shade_model", C.c_int32),
                ("shadow_samples", C.c_int32), ("seed", C.c_uint32), ("gamma", C.c_double),
                ("caustic_k", C.c_int32), ("caustic_radius", C.c_float), ("photon_count", C.c_int32), ("photon_bounce", C.c_int32)]


class _Sized(C.Structure):
    """a versioned struct the caller fills: its first field is struct_size, and the constructor writes it"""

    def __init__(self, **fields):
        super().__init__(struct_size=C.sizeof(type(self)), **fields)


class Outputs(_Sized):
    """rt_outputs: the planes of a render.  rgb8, z, count are required; the others are optional (NULL = not wanted)."""
    _fields_ = [("struct_size", C.c_uint32), ("rgb8", C.c_void_p), ("z", C.c_void_p), ("count", C.c_void_p),
                ("rgb_linear", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p), ("alpha", C.c_void_p),
                ("object_id", C.c_void_p)]


class DenoiseParams(C.Structure):
    """rt_denoise_params: the a-trous filter's parameters (rt_denoise_default_params fills 5 / 1.0 / 0.3 / 0.05 / 2.2)"""
    _fields_ = [("struct_size", C.c_uint32), ("levels", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_depth", C.c_float), ("gamma", C.c_float)]


class DenoisePlanes(_Sized):
    """rt_denoise_planes: the inputs and outputs of a denoise.  object_id and out_rgb8 are optional (NULL = not given)."""
    _fields_ = [("struct_size", C.c_uint32), ("rgb_linear", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p),
                ("z", C.c_void_p), ("object_id", C.c_void_p), ("out_linear", C.c_void_p), ("out_rgb8", C.c_void_p)]


class DenoiseVar(C.Structure):
    """rt_denoise_var: the variance block of the variance-guided denoise (rt_denoise_var_default fills k_sigma = 4.0).
    variance is required, out_variance optional (NULL = not wanted; may be `variance`)."""
    _fields_ = [("struct_size", C.c_uint32), ("variance", C.c_void_p), ("out_variance", C.c_void_p), ("k_sigma", C.c_float)]


class TemporalParams(C.Structure):
    """rt_temporal_params: the temporal accumulation's parameters (rt_temporal_default_params fills 0.2 / 32 / 0.3 / 0.05 / 2.2)"""
    _fields_ = [("struct_size", C.c_uint32), ("alpha", C.c_float), ("max_history", C.c_int32), ("sigma_normal", C.c_float),
                ("sigma_depth", C.c_float), ("gamma", C.c_float)]


class TemporalPlanes(_Sized):
    """rt_temporal_planes: the inputs and outputs of one accumulated frame.  object_id, variance, out_variance (needs variance),
    out_history and out_rgb8 are optional (NULL = not given)."""
    _fields_ = [("struct_size", C.c_uint32), ("rgb_linear", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p),
                ("z", C.c_void_p), ("object_id", C.c_void_p), ("variance", C.c_void_p), ("out_linear", C.c_void_p),
                ("out_variance", C.c_void_p), ("out_history", C.c_void_p), ("out_rgb8", C.c_void_p)]


class TemporalClip(C.Structure):
    """rt_temporal_clip: history rectification (rt_temporal_clip_default fills 2 / 1.5 / 4 / 2 and no out_clipped)"""
    _fields_ = [("struct_size", C.c_uint32), ("radius", C.c_int32), ("k_clip", C.c_float), ("min_count", C.c_int32),
                ("clip_history", C.c_int32), ("out_clipped", C.c_void_p)]


class MotionPlanes(_Sized):
    """rt_motion_planes: z and object_id of the new frame in, the motion plane (fx, fy, z_exp per pixel) out; all required"""
    _fields_ = [("struct_size", C.c_uint32), ("z", C.c_void_p), ("object_id", C.c_void_p), ("motion", C.c_void_p)]


class ToneMapParams(C.Structure):
    """rt_tonemap_params: exposure and tone mapping (rt_tonemap_default_params fills ACES, auto-exposure on, key 0.18, ev_bias 0,
    ev -16..16, percentiles 0.10..0.90, adapt 1 / 1, white 4, gamma 2.2)"""
    _fields_ = [("struct_size", C.c_uint32), ("op", C.c_int32), ("auto_exposure", C.c_int32), ("key", C.c_float), ("ev_bias", C.c_float),
                ("ev_min", C.c_float), ("ev_max", C.c_float), ("p_low", C.c_float), ("p_high", C.c_float), ("adapt_up", C.c_float),
                ("adapt_down", C.c_float), ("white", C.c_float), ("gamma", C.c_float)]


class ToneMapPlanes(_Sized):
    """rt_tonemap_planes: the input and outputs of one tone-mapped frame.  object_id is optional; one of out_display (may be
    rgb_linear) and out_rgb8 is required."""
    _fields_ = [("struct_size", C.c_uint32), ("rgb_linear", C.c_void_p), ("object_id", C.c_void_p), ("out_display", C.c_void_p),
                ("out_rgb8", C.c_void_p)]


class BloomParams(C.Structure):
    """rt_bloom_params: bloom ahead of tone mapping (rt_bloom_default_params fills threshold 1, knee 0.5, intensity 0.25, spread 0.7,
    levels 6, exposure_ev 0)"""
    _fields_ = [("struct_size", C.c_uint32), ("threshold", C.c_float), ("knee", C.c_float), ("intensity", C.c_float), ("spread", C.c_float),
                ("levels", C.c_int32), ("exposure_ev", C.c_float)]


class BloomPlanes(_Sized):
    """rt_bloom_planes: the input and outputs of one bloomed frame.  One of out (may be rgb_linear) and out_bloom is required."""
    _fields_ = [("struct_size", C.c_uint32), ("rgb_linear", C.c_void_p), ("out", C.c_void_p), ("out_bloom", C.c_void_p)]


class MotionBlurParams(C.Structure):
    """rt_motion_blur_params: motion blur between the denoise and bloom (rt_motion_blur_default_params fills shutter 0.5,
    max_blur 16, samples 15, depth_extent 0.05)"""
    _fields_ = [("struct_size", C.c_uint32), ("shutter", C.c_float), ("max_blur", C.c_int32), ("samples", C.c_int32),
                ("depth_extent", C.c_float)]


class MotionBlurPlanes(_Sized):
    """rt_motion_blur_planes: the inputs and outputs of one blurred frame.  out may not be rgb_linear; out_tiles is optional."""
    _fields_ = [("struct_size", C.c_uint32), ("rgb_linear", C.c_void_p), ("motion", C.c_void_p), ("z", C.c_void_p), ("out", C.c_void_p),
                ("out_tiles", C.c_void_p)]


class DofParams(C.Structure):
    """rt_dof_params: depth of field between the denoise and motion blur (rt_dof_default_params fills max_coc 16, samples 32,
    depth_extent 0.05, aperture_scale 1, focus 0 = the camera's focaldist)"""
    _fields_ = [("struct_size", C.c_uint32), ("max_coc", C.c_int32), ("samples", C.c_int32), ("depth_extent", C.c_float),
                ("aperture_scale", C.c_float), ("focus", C.c_float)]


class DofPlanes(_Sized):
    """rt_dof_planes: the inputs and outputs of one defocused frame.  out may not be rgb_linear; out_coc and out_tiles are optional."""
    _fields_ = [("struct_size", C.c_uint32), ("rgb_linear", C.c_void_p), ("z", C.c_void_p), ("out", C.c_void_p), ("out_coc", C.c_void_p),
                ("out_tiles", C.c_void_p)]


# rt_tonemap_params.op (include/rt_mi355x.h)
TONEMAP_CLAMP, TONEMAP_REINHARD, TONEMAP_ACES = 0, 1, 2
TONEMAP_OPERATORS = {"clamp": TONEMAP_CLAMP, "reinhard": TONEMAP_REINHARD, "aces": TONEMAP_ACES}

# the optional planes of Scene.render_outputs: name -> (rt_outputs field, dtype, channels).  "variance" is no field of rt_outputs:
# it is the extra argument of the _var entry points, which a render takes only when the plane is asked for
OUTPUT_PLANES = {"linear": ("rgb_linear", np.float32, 3), "normal": ("normal", np.float32, 3), "albedo": ("albedo", np.float32, 3),
                 "alpha": ("alpha", np.float32, 1), "object_id": ("object_id", np.int32, 1), "variance": (None, np.float32, 3)}
FEATURE_PLANES = ("normal", "albedo", "alpha", "object_id")
# the RT_PLANE_* bits of the packed planes format (rt_mi355x.h: "packed planes"), in the order of its sections behind the records
PLANE_BITS = {"linear": 1, "normal": 2, "albedo": 4, "alpha": 8, "object_id": 16, "variance": 32}
PACKED_SECTIONS = ("records", "normal", "albedo", "alpha", "object_id", "variance")


# one 128-byte node record of the tree the kernels walk (rt_scene_mesh_device_bvh): lo[axis][child], hi[axis][child], child refs
DEVBVHNODE = np.dtype([("lo", "<f4", (3, 4)), ("hi", "<f4", (3, 4)), ("c", "<u4", 4), ("pad", "<u4", 4)])
DEVBVH_LEAF = 0x80000000


class DeviceBvhInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_nodes", C.c_uint32), ("n_slots", C.c_uint32), ("root_ref", C.c_uint32),
                ("stack_need", C.c_int32), ("bvh_lds", C.c_int32), ("bvh_stack", C.c_int32), ("bvh_spill", C.c_int32),
                ("spill_blocks", C.c_int32), ("block", C.c_int32)]


class MeshUpdateMs(C.Structure):
    """rt_mesh_update_ms: the last in-place mesh update on a device, by events on the library's stream (milliseconds)"""
    _fields_ = [("struct_size", C.c_uint32), ("level_launches", C.c_int32), ("upload", C.c_float), ("retri", C.c_float), ("refit", C.c_float)]


class MeshQuality(C.Structure):
    """rt_mesh_quality: the SAH cost of a mesh's tree on a device against the cost it had when it was last built"""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("cost", C.c_double), ("built_cost", C.c_double),
                ("ratio", C.c_double), ("measure_ms", C.c_float)]

    def as_dict(self):
        return dict(cost=self.cost, built_cost=self.built_cost, ratio=self.ratio, measure_ms=self.measure_ms,
                    degenerate=bool(self.flags & MESH_QUALITY_DEGENERATE), rebuilt=bool(self.flags & MESH_QUALITY_REBUILT),
                    not_on_device=bool(self.flags & MESH_QUALITY_NOT_ON_DEVICE))


class MeshBuildInfo(C.Structure):
    """rt_mesh_build_info: what a device tree build reports (rt_scene_update_mesh_vertices_build)"""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_nodes", C.c_uint32), ("n_slots", C.c_uint32), ("root_ref", C.c_uint32),
                ("stack_need", C.c_int32), ("levels", C.c_int32), ("launches", C.c_int32), ("syncs", C.c_int32), ("pad", C.c_uint32),
                ("cost", C.c_double)] + [(n, C.c_float) for n in ("upload_ms", "sort_ms", "hierarchy_ms", "collapse_ms", "slots_ms", "cost_ms")]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n not in ("struct_size", "flags", "pad")}
        d.update(on_device=bool(self.flags & MESH_BUILD_ON_DEVICE), fell_back=bool(self.flags & MESH_BUILD_FELL_BACK),
                 not_on_device=bool(self.flags & MESH_BUILD_NOT_ON_DEVICE))
        return d


class MeshSkinInfo(C.Structure):
    """rt_mesh_skin_info: the skin bound to a mesh, and whether the store's positions are the last pose's (rt_scene_mesh_skin_info)"""
    _fields_ = [("struct_size", C.c_uint32), ("bound", C.c_uint32), ("n_bones", C.c_int32), ("nv", C.c_int32), ("store_current", C.c_uint32)]


class MeshMorphInfo(C.Structure):
    """rt_mesh_morph_info: the morph set bound to a mesh, and whether the store's positions are the last pose's (rt_scene_mesh_morph_info)"""
    _fields_ = [("struct_size", C.c_uint32), ("bound", C.c_uint32), ("n_targets", C.c_int32), ("nv", C.c_int32), ("store_current", C.c_uint32)]


class SetupMs(C.Structure):
    """rt_setup_ms: wall time of the stages of rt_scene_generate_photons, milliseconds"""
    _fields_ = [(n, C.c_double) for n in ("photon_pass", "balance", "structure_build", "upload", "total")]

    def as_dict(self):
        return {n: round(getattr(self, n), 3) for n, _ in self._fields_}


class TileRange(C.Structure):
    _fields_ = [("tile_w", C.c_int32), ("tile_h", C.c_int32), ("first", C.c_int32), ("stride", C.c_int32)]


class Stats(C.Structure):
    _fields_ = ([(n, C.c_uint64) for n in ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract",
                                           "instance_visits", "bvh_nodes_visited", "tris_tested",
                                           "photon_queries", "photons_visited", "pixels", "samples")] +
                [(n, C.c_double) for n in ("ms_trace", "ms_gather", "ms_resolve", "ms_total")] +
                [(n, C.c_uint64) for n in ("launches_trace", "launches_gather", "launches_resolve",
                                           "gather_rounds", "gather_slow", "gather_leaf_reads")] +
                [(n, C.c_double) for n in ("ms_primary", "ms_bounce")] +
                [(n, C.c_uint64) for n in ("launches_primary", "launches_bounce", "streams", "peak_rays", "peak_queries", "attempts")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# rt_scene_update_mesh_vertices flags (include/rt_mi355x.h): build the tree again instead of refitting it in place
MESH_UPDATE_REBUILD = 1
# ... and keep the positions the mesh had as its previous positions ("motion vectors for deforming meshes")
MESH_UPDATE_KEEP_PREVIOUS = 2
# rt_mesh_quality flags (include/rt_mi355x.h, "mesh tree quality")
MESH_QUALITY_DEGENERATE = 1
MESH_QUALITY_REBUILT = 2
MESH_QUALITY_NOT_ON_DEVICE = 4
# rt_mesh_build_info flags (include/rt_mi355x.h, "device tree build")
MESH_BUILD_ON_DEVICE = 1
MESH_BUILD_FELL_BACK = 2
MESH_BUILD_NOT_ON_DEVICE = 4
# rt_scene_set_mesh_normals_mode modes (include/rt_mi355x.h, "smooth normals")
MESH_NORMALS_STORED = 0
MESH_NORMALS_SMOOTH = 1

# the most bones a skin can have (include/rt_mi355x.h, "mesh skinning")
MESH_SKIN_MAX_BONES = 1024
# the most targets a morph set can have (include/rt_mi355x.h, "morph targets")
MESH_MORPH_MAX_TARGETS = 256

# rt_scene_set_render_flags bits (include/rt_mi355x.h): byte-identical renders for identical inputs
RENDER_REPRODUCIBLE = 1
# ... and the test hook that leaves every material's class word clear (FIN shading runs in full for every hit)
RENDER_GENERAL_SHADING = 4
# class bits of a material (rt_scene_material_classes; RT_MAT_* in csrc/rt_dev.h)
MAT_NO_SPEC_TREE = 1
MAT_NO_SPECULAR = 2


# Every function include/rt_mi355x.h declares, in the header's order: name -> (return type, parameter types).  A new ABI function
# is registered here and nowhere else; tests/test_host.py parses the header and fails on any entry that disagrees with it.
# int / int32_t -> i32, uint32_t -> u32, (u)int64_t -> i64 / u64, float / double -> f32 / f64, const char * -> text, every other
# pointer or array -> vp (byref(), ctypes arrays, addresses as int, None and c_void_p objects all pass); rt_status and int
# return as st.
st, vp, text = C.c_int, C.c_void_p, C.c_char_p
i32, u32, i64, u64, f32, f64 = C.c_int32, C.c_uint32, C.c_int64, C.c_uint64, C.c_float, C.c_double
SIGNATURES = {
    "rt_abi_version": (st, []),
    "rt_last_error": (text, []),
    "rt_device_count": (st, []),
    "rt_params_default": (None, [vp]),
    "rt_scene_create": (st, [vp]),
    "rt_scene_destroy": (None, [vp]),
    "rt_scene_set_nodes": (st, [vp, vp, i32]),
    "rt_scene_set_mesh": (st, [vp, i32, vp, i32, vp, i32, vp, i32, vp, vp, i32, vp]),
    "rt_scene_set_mesh_texcoords": (st, [vp, i32, vp, i32, vp]),
    "rt_scene_set_materials": (st, [vp, vp, i32]),
    "rt_scene_set_lights": (st, [vp, vp, i32]),
    "rt_scene_set_environment": (st, [vp, vp, vp]),
    "rt_scene_get_environment": (st, [vp, vp, vp]),
    "rt_scene_set_textures": (st, [vp, vp, i32, vp, u64]),
    "rt_scene_set_material_maps": (st, [vp, vp, i32]),
    "rt_scene_set_environment_maps": (st, [vp, vp, vp]),
    "rt_scene_get_textures": (st, [vp, vp, i32, vp, u64, vp, vp]),
    "rt_scene_get_maps": (st, [vp, vp, i32, vp, vp]),
    "rt_scene_set_photons": (st, [vp, vp, u32]),
    "rt_scene_set_caustic_photons": (st, [vp, vp, u32]),
    "rt_scene_load_xml": (st, [vp, text]),
    "rt_scene_get_camera": (st, [vp, vp]),
    "rt_scene_counts": (st, [vp, vp, vp, vp, vp, vp]),
    "rt_scene_get_nodes": (st, [vp, vp, i32]),
    "rt_scene_get_materials": (st, [vp, vp, i32]),
    "rt_scene_get_lights": (st, [vp, vp, i32]),
    "rt_scene_mesh_counts": (st, [vp, i32, vp, vp, vp, vp]),
    "rt_scene_get_mesh": (st, [vp, i32, vp, vp, vp, vp, vp, vp]),
    "rt_scene_get_mesh_texcoords": (st, [vp, i32, vp, vp, vp]),
    "rt_image_read_rgb": (st, [text, vp, vp, vp, u64]),
    "rt_image_write_png": (st, [text, vp, i32, i32, i32]),
    "rt_image_zbuffer": (st, [vp, i32, i32, vp]),
    "rt_image_write_pfm": (st, [text, vp, i32, i32]),
    "rt_image_read_pfm": (st, [text, vp, vp, vp, u64]),
    "rt_image_write_pfm1": (st, [text, vp, i32, i32]),
    "rt_image_read_pfm1": (st, [text, vp, vp, vp, u64]),
    "rt_image_sample_count": (st, [vp, i32, i32, vp, vp]),
    "rt_scene_generate_photons": (st, [vp, i32, u32, i32, u32, text, vp]),
    "rt_scene_set_photon_dump": (st, [vp, text]),
    "rt_scene_get_photons": (st, [vp, vp, u32, vp]),
    "rt_scene_mesh_device_bvh": (st, [vp, i32, vp, vp, u64, vp, u64]),
    "rt_scene_update_mesh_vertices": (st, [vp, i32, vp, i32, vp, i32, u32]),
    "rt_scene_update_mesh_vertices_flags": (st, [vp, i32, vp, i32, vp, i32, u32]),
    "rt_scene_mesh_device_read": (st, [vp, i32, i32, vp, vp, u64, vp, u64, vp, vp, vp]),
    "rt_scene_mesh_update_ms": (st, [vp, i32, vp]),
    "rt_device_bvh_cost": (st, [vp, u64, u32, vp, vp]),
    "rt_scene_mesh_quality": (st, [vp, i32, i32, vp]),
    "rt_scene_update_mesh_vertices_auto": (st, [vp, i32, vp, i32, vp, i32, f64, vp]),
    "rt_scene_update_mesh_vertices_auto_flags": (st, [vp, i32, vp, i32, vp, i32, f64, u32, vp]),
    "rt_scene_previous_positions": (st, [vp, vp]),
    "rt_scene_mesh_device_previous": (st, [vp, i32, i32, vp, u64, vp]),
    "rt_device_lbvh_build": (st, [vp, i32, vp, i32, vp, vp, u64, vp, u64]),
    "rt_scene_update_mesh_vertices_build": (st, [vp, i32, vp, i32, vp, i32, u32, vp]),
    "rt_scene_update_mesh_vertices_auto_build": (st, [vp, i32, vp, i32, vp, i32, f64, u32, vp, vp]),
    "rt_mesh_smooth_normals": (st, [vp, i32, vp, vp, i32, vp, i32]),
    "rt_scene_set_mesh_normals_mode": (st, [vp, i32, u32]),
    "rt_scene_get_mesh_normals_mode": (st, [vp, i32, vp]),
    "rt_scene_mesh_normals_ms": (st, [vp, i32, vp]),
    "rt_mesh_skin": (st, [vp, i32, vp, vp, vp, i32, vp]),
    "rt_scene_set_mesh_skin": (st, [vp, i32, i32, vp, vp, i32]),
    "rt_scene_clear_mesh_skin": (st, [vp, i32]),
    "rt_scene_mesh_skin_info": (st, [vp, i32, vp]),
    "rt_scene_pose_mesh": (st, [vp, i32, vp, i32, u32]),
    "rt_scene_pose_mesh_auto": (st, [vp, i32, vp, i32, u32, f64, vp]),
    "rt_scene_pose_mesh_build": (st, [vp, i32, vp, i32, u32, vp]),
    "rt_scene_pose_mesh_auto_build": (st, [vp, i32, vp, i32, u32, f64, vp, vp]),
    "rt_scene_mesh_skin_ms": (st, [vp, i32, vp]),
    "rt_mesh_morph": (st, [vp, i32, vp, i32, vp, vp]),
    "rt_scene_set_mesh_morphs": (st, [vp, i32, i32, vp, i32]),
    "rt_scene_clear_mesh_morphs": (st, [vp, i32]),
    "rt_scene_mesh_morph_info": (st, [vp, i32, vp]),
    "rt_scene_morph_mesh": (st, [vp, i32, vp, i32, vp, i32, u32]),
    "rt_scene_morph_mesh_auto": (st, [vp, i32, vp, i32, vp, i32, u32, f64, vp]),
    "rt_scene_morph_mesh_build": (st, [vp, i32, vp, i32, vp, i32, u32, vp]),
    "rt_scene_morph_mesh_auto_build": (st, [vp, i32, vp, i32, vp, i32, u32, f64, vp, vp]),
    "rt_scene_mesh_morph_ms": (st, [vp, i32, vp]),
    "rt_bvh_build": (st, [vp, i32, vp, i32, i32, vp, vp, vp]),
    "rt_photon_balance": (st, [vp, u32, vp]),
    "rt_photon_unreachable": (st, [vp, u32, vp, u32, vp]),
    "rt_photon_unreachable_device": (st, [i32, vp, u32, vp, u32, vp, vp]),
    "rt_photons_write_dat": (st, [text, vp, u32]),
    "rt_photons_read_dat": (st, [text, vp, u32, vp]),
    "rt_photon_pass": (st, [vp, i32, u32, i32, u32, vp, u32, vp, vp]),
    "rt_caustic_pass": (st, [vp, i32, u32, i32, u32, vp, u32, vp, vp]),
    "rt_scene_set_render_flags": (st, [vp, u32]),
    "rt_scene_get_render_flags": (st, [vp, vp]),
    "rt_scene_material_classes": (st, [vp, vp, i32, vp]),
    "rt_render_begin": (st, [vp, vp, vp, vp, i32, vp, vp, vp, vp]),
    "rt_render_tiles_device": (st, [vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp]),
    "rt_render_tiles_packed_device": (st, [vp, vp, vp, vp, i32, vp, vp, u64, i32, vp]),
    "rt_tiles_packed_size": (st, [i32, i32, vp, vp, vp]),
    "rt_tiles_unpack_device": (st, [i32, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp]),
    "rt_render_begin_linear": (st, [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]),
    "rt_render_tiles_linear_device": (st, [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp]),
    "rt_render_tiles_packed_linear_device": (st, [vp, vp, vp, vp, i32, vp, vp, u64, i32, vp]),
    "rt_tiles_unpack_linear_device": (st, [i32, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp]),
    "rt_render_begin_outputs": (st, [vp, vp, vp, vp, i32, vp, vp]),
    "rt_render_tiles_outputs_device": (st, [vp, vp, vp, vp, i32, vp, vp, i32, vp]),
    "rt_render_begin_outputs_var": (st, [vp, vp, vp, vp, i32, vp, vp, vp]),
    "rt_render_tiles_outputs_var_device": (st, [vp, vp, vp, vp, i32, vp, vp, vp, i32, vp]),
    "rt_tiles_packed_planes_size": (st, [i32, i32, vp, u32, vp, vp, vp]),
    "rt_render_tiles_packed_outputs_device": (st, [vp, vp, vp, vp, i32, vp, vp, u64, u32, i32, vp]),
    "rt_tiles_unpack_outputs_device": (st, [i32, vp, vp, i32, i32, i32, i32, i32, i32, u32, vp, vp]),
    "rt_render_check": (st, [vp, i32]),
    "rt_render_counters": (st, [vp, i32, i32, vp]),
    "rt_render_progress": (st, [vp]),
    "rt_render_stop": (st, [vp]),
    "rt_render_wait": (st, [vp]),
    "rt_job_stats": (st, [vp, vp]),
    "rt_job_setup_ms": (st, [vp, vp]),
    "rt_job_destroy": (None, [vp]),
    "rt_denoise_default_params": (None, [vp]),
    "rt_denoise_device": (st, [i32, vp, i32, i32, vp, vp, i32]),
    "rt_denoise": (st, [i32, i32, i32, vp, vp]),
    "rt_denoise_var_default": (None, [vp]),
    "rt_denoise_var_device": (st, [i32, vp, i32, i32, vp, vp, vp, i32]),
    "rt_denoise_var_host": (st, [i32, i32, i32, vp, vp, vp]),
    "rt_history_create": (st, [i32, i32, i32, vp]),
    "rt_history_reset": (st, [vp]),
    "rt_history_destroy": (None, [vp]),
    "rt_history_frames": (i32, [vp]),
    "rt_temporal_default_params": (None, [vp]),
    "rt_temporal_device": (st, [vp, vp, vp, vp, vp, i32]),
    "rt_temporal": (st, [vp, vp, vp, vp]),
    "rt_motion_device": (st, [i32, vp, vp, vp, vp, vp, i32, vp, i32]),
    "rt_motion": (st, [i32, vp, vp, vp, vp, i32, vp]),
    "rt_scene_motion_device": (st, [vp, i32, i32, vp, vp, vp, vp, i32, f32, vp, i32]),
    "rt_scene_motion": (st, [vp, i32, i32, vp, vp, vp, i32, f32, vp]),
    "rt_temporal_motion_device": (st, [vp, vp, vp, vp, vp, vp, i32]),
    "rt_temporal_motion": (st, [vp, vp, vp, vp, vp]),
    "rt_temporal_clip_default": (None, [vp]),
    "rt_temporal_clip_device": (st, [vp, vp, vp, vp, vp, vp, vp, i32]),
    "rt_temporal_clip_host": (st, [vp, vp, vp, vp, vp, vp]),
    "rt_exposure_create": (st, [i32, vp]),
    "rt_exposure_reset": (st, [vp]),
    "rt_exposure_destroy": (None, [vp]),
    "rt_exposure_get": (st, [vp, vp, vp, vp]),
    "rt_exposure_histogram": (st, [vp, vp]),
    "rt_tonemap_default_params": (None, [vp]),
    "rt_tonemap_device": (st, [vp, i32, vp, i32, i32, vp, vp, i32]),
    "rt_tonemap": (st, [vp, i32, i32, i32, vp, vp]),
    "rt_bloom_create": (st, [i32, i32, i32, vp]),
    "rt_bloom_destroy": (None, [vp]),
    "rt_bloom_default_params": (None, [vp]),
    "rt_bloom_plan": (st, [i32, i32, i32, vp, vp]),
    "rt_bloom_device": (st, [vp, vp, vp, vp, vp, i32]),
    "rt_bloom_host": (st, [vp, vp, vp, vp]),
    "rt_motion_blur_create": (st, [i32, i32, i32, vp]),
    "rt_motion_blur_destroy": (None, [vp]),
    "rt_motion_blur_default_params": (None, [vp]),
    "rt_motion_blur_tiles": (st, [i32, i32, i32, vp, vp]),
    "rt_motion_blur_device": (st, [vp, vp, vp, vp, i32]),
    "rt_motion_blur_host": (st, [vp, vp, vp]),
    "rt_dof_create": (st, [i32, i32, i32, vp]),
    "rt_dof_destroy": (None, [vp]),
    "rt_dof_default_params": (None, [vp]),
    "rt_dof_tiles": (st, [i32, i32, i32, vp, vp]),
    "rt_dof_taps": (st, [i32, vp]),
    "rt_dof_device": (st, [vp, vp, vp, vp, vp, i32]),
    "rt_dof_host": (st, [vp, vp, vp, vp]),
    "rt_trace_rays": (st, [vp, i32, i32, vp, i64, vp, vp, vp, vp, vp, vp]),
    "rt_estimate_irradiance": (st, [vp, i32, i32, f32, vp, vp, i64, vp, vp]),
    "rt_shade_rays": (st, [vp, vp, i32, vp, i64, vp, vp, vp]),
}
del st, vp, text, i32, u32, i64, u64, f32, f64
SYMBOLS = list(SIGNATURES)


class RtError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"rt_mi355x status {status}: {message}")
        self.status = status


def build(verbose=False):
    """Compile librt_mi355x.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-C", CSRC] + ([] if verbose else ["-s"]), check=True)


_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.environ.get("RT_MI355X_LIB", LIB_PATH)      # another build of the same ABI (tuning runs)
        if not os.path.exists(path):
            raise RtError(-3, f"{path} is missing: run __graft_entry__.build() (no CPU fallback exists)")
        loaded = C.CDLL(path)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(loaded, name)          # AttributeError here = header/library mismatch
            fn.restype, fn.argtypes = restype, argtypes
        _lib = loaded
    return _lib


def _check(status):
    if status != 0:
        raise RtError(status, lib().rt_last_error().decode(errors="replace"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def _c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _stream_handle(stream):
    if stream is None:
        return None
    if int(stream) == 0:
        raise ValueError("stream handle 0 (torch's legacy default stream) cannot be named here: NULL means the library's own "
                         "stream; use an explicit torch.cuda.Stream")
    return C.c_void_p(int(stream))


class _Handle:
    """what the classes that own a library object share: self._h is its handle, made by the library function the subclass names in
    _create from the device and the size (kept under the attribute names in _size); close() (or the end of a with block, or the
    collector) hands it to the one named in _destroy"""
    _create = _destroy = None
    _size = ()

    def __init__(self, device, *size):
        if len(size) != len(self._size):
            raise TypeError(f"{type(self).__name__} takes a device and {len(self._size)} size arguments, {len(size)} were given")
        self._h = C.c_void_p()
        self.device = int(device)
        for name, v in zip(self._size, size):
            setattr(self, name, int(v))
        _check(getattr(lib(), self._create)(self.device, *(getattr(self, name) for name in self._size), C.byref(self._h)))

    def close(self):
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
