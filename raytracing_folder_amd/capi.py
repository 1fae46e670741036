"""ctypes binding of librt_mi355x.so (the C ABI declared in include/rt_mi355x.h).

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


class Outputs(C.Structure):
    """rt_outputs: the planes of a render.  rgb8, z, count are required; the others are optional (NULL = not wanted)."""
    _fields_ = [("struct_size", C.c_uint32), ("rgb8", C.c_void_p), ("z", C.c_void_p), ("count", C.c_void_p),
                ("rgb_linear", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p), ("alpha", C.c_void_p),
                ("object_id", C.c_void_p)]

    def __init__(self, **planes):
        super().__init__(struct_size=C.sizeof(Outputs), **planes)


class DenoiseParams(C.Structure):
    """rt_denoise_params: the a-trous filter's parameters (rt_denoise_default_params fills 5 / 1.0 / 0.3 / 0.05 / 2.2)"""
    _fields_ = [("struct_size", C.c_uint32), ("levels", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_depth", C.c_float), ("gamma", C.c_float)]


class DenoisePlanes(C.Structure):
    """rt_denoise_planes: the inputs and outputs of a denoise.  object_id and out_rgb8 are optional (NULL = not given)."""
    _fields_ = [("struct_size", C.c_uint32), ("rgb_linear", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p),
                ("z", C.c_void_p), ("object_id", C.c_void_p), ("out_linear", C.c_void_p), ("out_rgb8", C.c_void_p)]

    def __init__(self, **planes):
        super().__init__(struct_size=C.sizeof(DenoisePlanes), **planes)


class DenoiseVar(C.Structure):
    """rt_denoise_var: the variance block of the variance-guided denoise (rt_denoise_var_default fills k_sigma = 4.0).
    variance is required, out_variance optional (NULL = not wanted; may be `variance`)."""
    _fields_ = [("struct_size", C.c_uint32), ("variance", C.c_void_p), ("out_variance", C.c_void_p), ("k_sigma", C.c_float)]


class TemporalParams(C.Structure):
    """rt_temporal_params: the temporal accumulation's parameters (rt_temporal_default_params fills 0.2 / 32 / 0.3 / 0.05 / 2.2)"""
    _fields_ = [("struct_size", C.c_uint32), ("alpha", C.c_float), ("max_history", C.c_int32), ("sigma_normal", C.c_float),
                ("sigma_depth", C.c_float), ("gamma", C.c_float)]


class TemporalPlanes(C.Structure):
    """rt_temporal_planes: the inputs and outputs of one accumulated frame.  object_id, variance, out_variance (needs variance),
    out_history and out_rgb8 are optional (NULL = not given)."""
    _fields_ = [("struct_size", C.c_uint32), ("rgb_linear", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p),
                ("z", C.c_void_p), ("object_id", C.c_void_p), ("variance", C.c_void_p), ("out_linear", C.c_void_p),
                ("out_variance", C.c_void_p), ("out_history", C.c_void_p), ("out_rgb8", C.c_void_p)]

    def __init__(self, **planes):
        super().__init__(struct_size=C.sizeof(TemporalPlanes), **planes)


class TemporalClip(C.Structure):
    """rt_temporal_clip: history rectification (rt_temporal_clip_default fills 2 / 1.5 / 4 / 2 and no out_clipped)"""
    _fields_ = [("struct_size", C.c_uint32), ("radius", C.c_int32), ("k_clip", C.c_float), ("min_count", C.c_int32),
                ("clip_history", C.c_int32), ("out_clipped", C.c_void_p)]


class MotionPlanes(C.Structure):
    """rt_motion_planes: z and object_id of the new frame in, the motion plane (fx, fy, z_exp per pixel) out; all required"""
    _fields_ = [("struct_size", C.c_uint32), ("z", C.c_void_p), ("object_id", C.c_void_p), ("motion", C.c_void_p)]

    def __init__(self, **planes):
        super().__init__(struct_size=C.sizeof(MotionPlanes), **planes)


class ToneMapParams(C.Structure):
    """rt_tonemap_params: exposure and tone mapping (rt_tonemap_default_params fills ACES, auto-exposure on, key 0.18, ev_bias 0,
    ev -16..16, percentiles 0.10..0.90, adapt 1 / 1, white 4, gamma 2.2)"""
    _fields_ = [("struct_size", C.c_uint32), ("op", C.c_int32), ("auto_exposure", C.c_int32), ("key", C.c_float), ("ev_bias", C.c_float),
                ("ev_min", C.c_float), ("ev_max", C.c_float), ("p_low", C.c_float), ("p_high", C.c_float), ("adapt_up", C.c_float),
                ("adapt_down", C.c_float), ("white", C.c_float), ("gamma", C.c_float)]


class ToneMapPlanes(C.Structure):
    """rt_tonemap_planes: the input and outputs of one tone-mapped frame.  object_id is optional; one of out_display (may be
    rgb_linear) and out_rgb8 is required."""
    _fields_ = [("struct_size", C.c_uint32), ("rgb_linear", C.c_void_p), ("object_id", C.c_void_p), ("out_display", C.c_void_p),
                ("out_rgb8", C.c_void_p)]

    def __init__(self, **planes):
        super().__init__(struct_size=C.sizeof(ToneMapPlanes), **planes)


class BloomParams(C.Structure):
    """rt_bloom_params: bloom ahead of tone mapping (rt_bloom_default_params fills threshold 1, knee 0.5, intensity 0.25, spread 0.7,
    levels 6, exposure_ev 0)"""
    _fields_ = [("struct_size", C.c_uint32), ("threshold", C.c_float), ("knee", C.c_float), ("intensity", C.c_float), ("spread", C.c_float),
                ("levels", C.c_int32), ("exposure_ev", C.c_float)]


class BloomPlanes(C.Structure):
    """rt_bloom_planes: the input and outputs of one bloomed frame.  One of out (may be rgb_linear) and out_bloom is required."""
    _fields_ = [("struct_size", C.c_uint32), ("rgb_linear", C.c_void_p), ("out", C.c_void_p), ("out_bloom", C.c_void_p)]

    def __init__(self, **planes):
        super().__init__(struct_size=C.sizeof(BloomPlanes), **planes)


class MotionBlurParams(C.Structure):
    """rt_motion_blur_params: motion blur between the denoise and bloom (rt_motion_blur_default_params fills shutter 0.5,
    max_blur 16, samples 15, depth_extent 0.05)"""
    _fields_ = [("struct_size", C.c_uint32), ("shutter", C.c_float), ("max_blur", C.c_int32), ("samples", C.c_int32),
                ("depth_extent", C.c_float)]


class MotionBlurPlanes(C.Structure):
    """rt_motion_blur_planes: the inputs and outputs of one blurred frame.  out may not be rgb_linear; out_tiles is optional."""
    _fields_ = [("struct_size", C.c_uint32), ("rgb_linear", C.c_void_p), ("motion", C.c_void_p), ("z", C.c_void_p), ("out", C.c_void_p),
                ("out_tiles", C.c_void_p)]

    def __init__(self, **planes):
        super().__init__(struct_size=C.sizeof(MotionBlurPlanes), **planes)


class DofParams(C.Structure):
    """rt_dof_params: depth of field between the denoise and motion blur (rt_dof_default_params fills max_coc 16, samples 32,
    depth_extent 0.05, aperture_scale 1, focus 0 = the camera's focaldist)"""
    _fields_ = [("struct_size", C.c_uint32), ("max_coc", C.c_int32), ("samples", C.c_int32), ("depth_extent", C.c_float),
                ("aperture_scale", C.c_float), ("focus", C.c_float)]


class DofPlanes(C.Structure):
    """rt_dof_planes: the inputs and outputs of one defocused frame.  out may not be rgb_linear; out_coc and out_tiles are optional."""
    _fields_ = [("struct_size", C.c_uint32), ("rgb_linear", C.c_void_p), ("z", C.c_void_p), ("out", C.c_void_p), ("out_coc", C.c_void_p),
                ("out_tiles", C.c_void_p)]

    def __init__(self, **planes):
        super().__init__(struct_size=C.sizeof(DofPlanes), **planes)


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


# every symbol include/rt_mi355x.h declares
SYMBOLS = [
    "rt_abi_version", "rt_last_error", "rt_device_count", "rt_params_default",
    "rt_scene_create", "rt_scene_destroy", "rt_scene_set_nodes", "rt_scene_set_mesh",
    "rt_scene_set_mesh_texcoords", "rt_scene_get_mesh_texcoords",
    "rt_scene_set_materials", "rt_scene_set_lights", "rt_scene_set_environment", "rt_scene_get_environment",
    "rt_scene_set_photons", "rt_scene_set_caustic_photons", "rt_scene_set_textures", "rt_scene_set_material_maps", "rt_scene_set_environment_maps",
    "rt_scene_get_textures", "rt_scene_get_maps", "rt_image_read_rgb", "rt_image_write_png", "rt_image_zbuffer", "rt_image_sample_count", "rt_scene_load_xml", "rt_scene_get_camera", "rt_scene_counts",
    "rt_scene_get_nodes", "rt_scene_get_materials", "rt_scene_get_lights", "rt_scene_mesh_counts",
    "rt_scene_get_mesh", "rt_bvh_build", "rt_photon_balance", "rt_photons_write_dat", "rt_photons_read_dat", "rt_photon_pass", "rt_caustic_pass", "rt_render_begin",
    "rt_render_tiles_device", "rt_render_tiles_packed_device", "rt_tiles_packed_size", "rt_tiles_unpack_device", "rt_render_check", "rt_render_counters", "rt_render_progress", "rt_render_stop", "rt_render_wait",
    "rt_job_stats", "rt_job_setup_ms", "rt_job_destroy", "rt_trace_rays", "rt_estimate_irradiance", "rt_shade_rays",
    "rt_scene_generate_photons", "rt_scene_set_photon_dump", "rt_scene_get_photons", "rt_photon_unreachable", "rt_photon_unreachable_device",
    "rt_scene_set_render_flags", "rt_scene_get_render_flags",
    "rt_render_begin_linear", "rt_render_tiles_linear_device", "rt_render_tiles_packed_linear_device", "rt_tiles_unpack_linear_device",
    "rt_image_write_pfm", "rt_image_read_pfm",
    "rt_render_begin_outputs", "rt_render_tiles_outputs_device", "rt_image_write_pfm1", "rt_image_read_pfm1",
    "rt_denoise_default_params", "rt_denoise_device", "rt_denoise",
    "rt_render_begin_outputs_var", "rt_render_tiles_outputs_var_device",
    "rt_denoise_var_default", "rt_denoise_var_device", "rt_denoise_var_host",
    "rt_history_create", "rt_history_reset", "rt_history_destroy", "rt_history_frames",
    "rt_temporal_default_params", "rt_temporal_device", "rt_temporal",
    "rt_motion_device", "rt_motion", "rt_temporal_motion_device", "rt_temporal_motion",
    "rt_temporal_clip_default", "rt_temporal_clip_device", "rt_temporal_clip_host",
    "rt_exposure_create", "rt_exposure_reset", "rt_exposure_destroy", "rt_exposure_get", "rt_exposure_histogram",
    "rt_tonemap_default_params", "rt_tonemap_device", "rt_tonemap",
    "rt_bloom_create", "rt_bloom_destroy", "rt_bloom_default_params", "rt_bloom_plan", "rt_bloom_device", "rt_bloom_host",
    "rt_motion_blur_create", "rt_motion_blur_destroy", "rt_motion_blur_default_params", "rt_motion_blur_tiles", "rt_motion_blur_device",
    "rt_motion_blur_host",
    "rt_dof_create", "rt_dof_destroy", "rt_dof_default_params", "rt_dof_tiles", "rt_dof_taps", "rt_dof_device", "rt_dof_host",
    "rt_tiles_packed_planes_size", "rt_render_tiles_packed_outputs_device", "rt_tiles_unpack_outputs_device",
    "rt_scene_mesh_device_bvh",
    "rt_scene_update_mesh_vertices", "rt_scene_mesh_device_read", "rt_scene_mesh_update_ms",
    "rt_scene_material_classes",
    "rt_device_bvh_cost", "rt_scene_mesh_quality", "rt_scene_update_mesh_vertices_auto",
    "rt_scene_update_mesh_vertices_flags", "rt_scene_update_mesh_vertices_auto_flags", "rt_scene_previous_positions", "rt_scene_mesh_device_previous",
    "rt_scene_motion_device", "rt_scene_motion",
]

# rt_scene_update_mesh_vertices flags (include/rt_mi355x.h): build the tree again instead of refitting it in place
MESH_UPDATE_REBUILD = 1
# ... and keep the positions the mesh had as its previous positions ("motion vectors for deforming meshes")
MESH_UPDATE_KEEP_PREVIOUS = 2
# rt_mesh_quality flags (include/rt_mi355x.h, "mesh tree quality")
MESH_QUALITY_DEGENERATE = 1
MESH_QUALITY_REBUILT = 2
MESH_QUALITY_NOT_ON_DEVICE = 4

# rt_scene_set_render_flags bits (include/rt_mi355x.h): byte-identical renders for identical inputs
RENDER_REPRODUCIBLE = 1
# ... and the test hook that leaves every material's class word clear (FIN shading runs in full for every hit)
RENDER_GENERAL_SHADING = 4
# class bits of a material (rt_scene_material_classes; RT_MAT_* in csrc/rt_dev.h)
MAT_NO_SPEC_TREE = 1
MAT_NO_SPECULAR = 2


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
        _lib = C.CDLL(path)
        _lib.rt_last_error.restype = C.c_char_p
        for name in SYMBOLS:
            getattr(_lib, name)          # AttributeError here = header/library mismatch
        _lib.rt_render_progress.restype = C.c_int
        _lib.rt_scene_set_render_flags.argtypes = [C.c_void_p, C.c_uint32]
        _lib.rt_scene_set_render_flags.restype = C.c_int
        _lib.rt_scene_get_render_flags.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        _lib.rt_scene_get_render_flags.restype = C.c_int
        _lib.rt_scene_material_classes.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        _lib.rt_scene_material_classes.restype = C.c_int
        # the linear plane (rt_mi355x.h: "the linear plane")
        vp, i32 = C.c_void_p, C.c_int32
        _lib.rt_render_begin_linear.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]
        _lib.rt_render_tiles_linear_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp]
        _lib.rt_render_tiles_packed_linear_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, C.c_uint64, C.c_int, vp]
        _lib.rt_tiles_unpack_linear_device.argtypes = [C.c_int, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp]
        _lib.rt_image_write_pfm.argtypes = [C.c_char_p, vp, i32, i32]
        _lib.rt_image_read_pfm.argtypes = [C.c_char_p, C.POINTER(i32), C.POINTER(i32), vp, C.c_uint64]
        # the plane descriptor and the first-hit feature planes (rt_mi355x.h: "first-hit feature planes")
        _lib.rt_render_begin_outputs.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp]
        _lib.rt_render_tiles_outputs_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp]
        _lib.rt_image_write_pfm1.argtypes = [C.c_char_p, vp, i32, i32]
        _lib.rt_image_read_pfm1.argtypes = [C.c_char_p, C.POINTER(i32), C.POINTER(i32), vp, C.c_uint64]
        # the denoiser (rt_mi355x.h: "denoising")
        _lib.rt_denoise_default_params.argtypes = [vp]
        _lib.rt_denoise_default_params.restype = None
        _lib.rt_denoise_device.argtypes = [C.c_int, vp, i32, i32, vp, vp, C.c_int]
        _lib.rt_denoise.argtypes = [C.c_int, i32, i32, vp, vp]
        _lib.rt_denoise_device.restype = _lib.rt_denoise.restype = C.c_int
        # the variance plane and the variance-guided denoise (rt_mi355x.h: "the variance plane", "variance-guided denoising")
        _lib.rt_render_begin_outputs_var.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp]
        _lib.rt_render_tiles_outputs_var_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, vp]
        _lib.rt_denoise_var_default.argtypes = [vp]
        _lib.rt_denoise_var_default.restype = None
        _lib.rt_denoise_var_device.argtypes = [C.c_int, vp, i32, i32, vp, vp, vp, C.c_int]
        _lib.rt_denoise_var_host.argtypes = [C.c_int, i32, i32, vp, vp, vp]
        for name in ("rt_render_begin_outputs_var", "rt_render_tiles_outputs_var_device", "rt_denoise_var_device", "rt_denoise_var_host"):
            getattr(_lib, name).restype = C.c_int
        # temporal accumulation (rt_mi355x.h: "temporal accumulation")
        _lib.rt_history_create.argtypes = [C.c_int, i32, i32, C.POINTER(vp)]
        _lib.rt_history_reset.argtypes = [vp]
        _lib.rt_history_destroy.argtypes = [vp]
        _lib.rt_history_destroy.restype = None
        _lib.rt_history_frames.argtypes = [vp]
        _lib.rt_history_frames.restype = i32
        _lib.rt_temporal_default_params.argtypes = [vp]
        _lib.rt_temporal_default_params.restype = None
        _lib.rt_temporal_device.argtypes = [vp, vp, vp, vp, vp, C.c_int]
        _lib.rt_temporal.argtypes = [vp, vp, vp, vp]
        for name in ("rt_history_create", "rt_history_reset", "rt_temporal_device", "rt_temporal"):
            getattr(_lib, name).restype = C.c_int
        # motion vectors (rt_mi355x.h: "motion vectors")
        _lib.rt_motion_device.argtypes = [C.c_int, vp, vp, vp, vp, vp, i32, vp, C.c_int]
        _lib.rt_motion.argtypes = [C.c_int, vp, vp, vp, vp, i32, vp]
        _lib.rt_temporal_motion_device.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int]
        _lib.rt_temporal_motion.argtypes = [vp, vp, vp, vp, vp]
        for name in ("rt_motion_device", "rt_motion", "rt_temporal_motion_device", "rt_temporal_motion"):
            getattr(_lib, name).restype = C.c_int
        # history rectification (rt_mi355x.h: "history rectification")
        _lib.rt_temporal_clip_default.argtypes = [vp]
        _lib.rt_temporal_clip_default.restype = None
        _lib.rt_temporal_clip_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_int]
        _lib.rt_temporal_clip_host.argtypes = [vp, vp, vp, vp, vp, vp]
        _lib.rt_temporal_clip_device.restype = _lib.rt_temporal_clip_host.restype = C.c_int
        # exposure and tone mapping (rt_mi355x.h: "exposure and tone mapping")
        _lib.rt_exposure_create.argtypes = [C.c_int, C.POINTER(vp)]
        _lib.rt_exposure_reset.argtypes = [vp]
        _lib.rt_exposure_destroy.argtypes = [vp]
        _lib.rt_exposure_destroy.restype = None
        _lib.rt_exposure_get.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
        _lib.rt_exposure_histogram.argtypes = [vp, vp]
        _lib.rt_tonemap_default_params.argtypes = [vp]
        _lib.rt_tonemap_default_params.restype = None
        _lib.rt_tonemap_device.argtypes = [vp, C.c_int, vp, i32, i32, vp, vp, C.c_int]
        _lib.rt_tonemap.argtypes = [vp, C.c_int, i32, i32, vp, vp]
        for name in ("rt_exposure_create", "rt_exposure_reset", "rt_exposure_get", "rt_exposure_histogram", "rt_tonemap_device", "rt_tonemap"):
            getattr(_lib, name).restype = C.c_int
        # bloom (rt_mi355x.h: "bloom")
        _lib.rt_bloom_create.argtypes = [C.c_int, i32, i32, C.POINTER(vp)]
        _lib.rt_bloom_destroy.argtypes = [vp]
        _lib.rt_bloom_destroy.restype = None
        _lib.rt_bloom_default_params.argtypes = [vp]
        _lib.rt_bloom_default_params.restype = None
        _lib.rt_bloom_plan.argtypes = [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
        _lib.rt_bloom_device.argtypes = [vp, vp, vp, vp, vp, C.c_int]
        _lib.rt_bloom_host.argtypes = [vp, vp, vp, vp]
        for name in ("rt_bloom_create", "rt_bloom_plan", "rt_bloom_device", "rt_bloom_host"):
            getattr(_lib, name).restype = C.c_int
        # motion blur (rt_mi355x.h: "motion blur")
        _lib.rt_motion_blur_create.argtypes = [C.c_int, i32, i32, C.POINTER(vp)]
        _lib.rt_motion_blur_destroy.argtypes = [vp]
        _lib.rt_motion_blur_destroy.restype = None
        _lib.rt_motion_blur_default_params.argtypes = [vp]
        _lib.rt_motion_blur_default_params.restype = None
        _lib.rt_motion_blur_tiles.argtypes = [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
        _lib.rt_motion_blur_device.argtypes = [vp, vp, vp, vp, C.c_int]
        _lib.rt_motion_blur_host.argtypes = [vp, vp, vp]
        for name in ("rt_motion_blur_create", "rt_motion_blur_tiles", "rt_motion_blur_device", "rt_motion_blur_host"):
            getattr(_lib, name).restype = C.c_int
        # depth of field (rt_mi355x.h: "depth of field")
        _lib.rt_dof_create.argtypes = [C.c_int, i32, i32, C.POINTER(vp)]
        _lib.rt_dof_destroy.argtypes = [vp]
        _lib.rt_dof_destroy.restype = None
        _lib.rt_dof_default_params.argtypes = [vp]
        _lib.rt_dof_default_params.restype = None
        _lib.rt_dof_tiles.argtypes = [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
        _lib.rt_dof_taps.argtypes = [i32, vp]
        _lib.rt_dof_device.argtypes = [vp, vp, vp, vp, vp, C.c_int]
        _lib.rt_dof_host.argtypes = [vp, vp, vp, vp]
        for name in ("rt_dof_create", "rt_dof_tiles", "rt_dof_taps", "rt_dof_device", "rt_dof_host"):
            getattr(_lib, name).restype = C.c_int
        # the packed planes of the multi-GPU exchange (rt_mi355x.h: "packed planes")
        _lib.rt_tiles_packed_planes_size.argtypes = [i32, i32, vp, C.c_uint32, vp, vp, vp]
        _lib.rt_render_tiles_packed_outputs_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, C.c_uint64, C.c_uint32, C.c_int, vp]
        _lib.rt_tiles_unpack_outputs_device.argtypes = [C.c_int, vp, vp, i32, i32, i32, i32, i32, i32, C.c_uint32, vp, vp]
        for name in ("rt_tiles_packed_planes_size", "rt_render_tiles_packed_outputs_device", "rt_tiles_unpack_outputs_device"):
            getattr(_lib, name).restype = C.c_int
        # the device tree of a mesh, on the host (rt_mi355x.h: rt_scene_mesh_device_bvh)
        _lib.rt_scene_mesh_device_bvh.argtypes = [vp, i32, vp, vp, C.c_uint64, vp, C.c_uint64]
        _lib.rt_scene_mesh_device_bvh.restype = C.c_int
        # mesh vertex updates (rt_mi355x.h: "mesh vertex updates")
        _lib.rt_scene_update_mesh_vertices.argtypes = [vp, i32, vp, i32, vp, i32, C.c_uint32]
        _lib.rt_scene_mesh_device_read.argtypes = [vp, C.c_int, i32, vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp]
        _lib.rt_scene_mesh_update_ms.argtypes = [vp, C.c_int, vp]
        for name in ("rt_scene_update_mesh_vertices", "rt_scene_mesh_device_read", "rt_scene_mesh_update_ms"):
            getattr(_lib, name).restype = C.c_int
        # mesh tree quality (rt_mi355x.h: "mesh tree quality")
        _lib.rt_device_bvh_cost.argtypes = [vp, C.c_uint64, C.c_uint32, vp, vp]
        _lib.rt_scene_mesh_quality.argtypes = [vp, C.c_int, i32, vp]
        _lib.rt_scene_update_mesh_vertices_auto.argtypes = [vp, i32, vp, i32, vp, i32, C.c_double, vp]
        for name in ("rt_device_bvh_cost", "rt_scene_mesh_quality", "rt_scene_update_mesh_vertices_auto"):
            getattr(_lib, name).restype = C.c_int
        # motion vectors for deforming meshes (rt_mi355x.h)
        _lib.rt_scene_update_mesh_vertices_flags.argtypes = [vp, i32, vp, i32, vp, i32, C.c_uint32]
        _lib.rt_scene_update_mesh_vertices_auto_flags.argtypes = [vp, i32, vp, i32, vp, i32, C.c_double, C.c_uint32, vp]
        _lib.rt_scene_previous_positions.argtypes = [vp, C.POINTER(i32)]
        _lib.rt_scene_mesh_device_previous.argtypes = [vp, C.c_int, i32, vp, C.c_uint64, C.POINTER(C.c_uint32)]
        _lib.rt_scene_motion_device.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, i32, C.c_float, vp, C.c_int]
        _lib.rt_scene_motion.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, i32, C.c_float, vp]
        for name in ("rt_scene_update_mesh_vertices_flags", "rt_scene_update_mesh_vertices_auto_flags", "rt_scene_previous_positions", "rt_scene_mesh_device_previous",
                     "rt_scene_motion_device", "rt_scene_motion"):
            getattr(_lib, name).restype = C.c_int
        for name in ("rt_render_begin_linear", "rt_render_tiles_linear_device", "rt_render_tiles_packed_linear_device",
                     "rt_tiles_unpack_linear_device", "rt_image_write_pfm", "rt_image_read_pfm",
                     "rt_render_begin_outputs", "rt_render_tiles_outputs_device", "rt_image_write_pfm1", "rt_image_read_pfm1"):
            getattr(_lib, name).restype = C.c_int
    return _lib


def _check(st):
    if st != 0:
        raise RtError(st, lib().rt_last_error().decode(errors="replace"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def _c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def device_bvh_cost(nodes, root_ref):
    """rt_device_bvh_cost, the host mirror of k_bvh_cost (no GPU): (cost, degenerate) of DEVBVHNODE records and their root ref"""
    nodes = _c(nodes, DEVBVHNODE)
    cost, flags = C.c_double(0.0), C.c_uint32(0)
    _check(lib().rt_device_bvh_cost(_p(nodes), len(nodes), C.c_uint32(int(root_ref)), C.byref(cost), C.byref(flags)))
    return cost.value, bool(flags.value & MESH_QUALITY_DEGENERATE)


def _stream_handle(stream):
    if stream is None:
        return None
    if int(stream) == 0:
        raise ValueError("stream handle 0 (torch's legacy default stream) cannot be named here: NULL means the library's own "
                         "stream; use an explicit torch.cuda.Stream")
    return C.c_void_p(int(stream))


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
    _check(lib().rt_image_read_rgb(os.fsencode(path), C.byref(w), C.byref(h), None, C.c_uint64(0)))
    rgb = np.zeros((h.value, w.value, 3), np.uint8)
    _check(lib().rt_image_read_rgb(os.fsencode(path), C.byref(w), C.byref(h), _p(rgb), C.c_uint64(rgb.size)))
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
    handle = _stream_handle(stream)
    args = (int(device), handle, C.c_void_p(gathered_ptr), int(world), int(tiles_per_rank), int(width), int(height), int(tile_w),
            int(tile_h), C.c_void_p(rgb_ptr), C.c_void_p(z_ptr), C.c_void_p(cnt_ptr))
    if linear_ptr is None:
        _check(lib().rt_tiles_unpack_device(*args))
    else:
        _check(lib().rt_tiles_unpack_linear_device(*args, C.c_void_p(linear_ptr)))


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
    _check(lib().rt_tiles_unpack_outputs_device(int(device), _stream_handle(stream), C.c_void_p(gathered_ptr), int(world), int(tiles_per_rank),
                                                int(width), int(height), int(tile_w), int(tile_h), plane_mask(planes), C.byref(o),
                                                C.c_void_p(variance_ptr) if variance_ptr is not None else None))


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


def _fill_params(struct, default_fn, allowed, int_fields, kw, what):
    """a `struct` as the library's `default_fn` fills it, then the keywords `kw` (of `allowed`; `int_fields` through int())"""
    p = struct()
    getattr(lib(), default_fn)(C.byref(p))
    for k, v in kw.items():
        if k not in allowed:
            raise TypeError(f"no {what} parameter {k!r}")
        setattr(p, k, int(v) if k in int_fields else v)
    return p


def denoise_params(**kw):
    """rt_denoise_default_params, then the keywords (levels, sigma_color, sigma_normal, sigma_depth, gamma)"""
    return _fill_params(DenoiseParams, "rt_denoise_default_params", ("levels", "sigma_color", "sigma_normal", "sigma_depth", "gamma"), (), kw, "denoise")


def denoise_var(variance_ptr, out_variance_ptr=None, k_sigma=4.0):
    """rt_denoise_var_default, then the two planes (addresses) and k_sigma"""
    v = DenoiseVar()
    lib().rt_denoise_var_default(C.byref(v))
    v.variance, v.out_variance, v.k_sigma = variance_ptr, out_variance_ptr, k_sigma
    return v


def denoise(linear, normal, albedo, z, object_id=None, rgb8=False, device=0, variance=None, k_sigma=4.0, return_variance=False, **params):
    """The a-trous denoise of a linear frame (rt_denoise; the definition: rt_mi355x.h, "denoising") on host arrays: float32
    (H, W, 3) linear / normal / albedo, float32 (H, W) z, optionally int32 (H, W) object_id.  Returns the denoised float32
    (H, W, 3) array -- with rgb8=True the pair (denoised, its gamma-encoded uint8 (H, W, 3) image).  params: denoise_params().
    variance (float32 (H, W, 3), the variance plane of the render): the variance-guided filter (rt_denoise_var_host) with a colour
    tolerance of k_sigma standard errors per pixel; return_variance=True appends the filtered variance (H, W, 3) to the result."""
    linear, normal, albedo = (_c(a, np.float32) for a in (linear, normal, albedo))
    h, w = linear.shape[:2]
    z = _c(z, np.float32)
    ids = _c(object_id, np.int32) if object_id is not None else None
    assert linear.shape == normal.shape == albedo.shape == (h, w, 3) and z.shape == (h, w) and (ids is None or ids.shape == (h, w))
    out = np.empty((h, w, 3), np.float32)
    out8 = np.empty((h, w, 3), np.uint8) if rgb8 else None
    pl = DenoisePlanes(rgb_linear=linear.ctypes.data, normal=normal.ctypes.data, albedo=albedo.ctypes.data, z=z.ctypes.data,
                       object_id=ids.ctypes.data if ids is not None else None, out_linear=out.ctypes.data,
                       out_rgb8=out8.ctypes.data if rgb8 else None)
    p = denoise_params(**params)
    if variance is None:
        if return_variance:
            raise TypeError("return_variance needs a variance plane")
        _check(lib().rt_denoise(int(device), w, h, C.byref(p), C.byref(pl)))
        return (out, out8) if rgb8 else out
    variance = _c(variance, np.float32)
    assert variance.shape == (h, w, 3)
    out_var = np.empty((h, w, 3), np.float32) if return_variance else None
    v = denoise_var(variance.ctypes.data, out_var.ctypes.data if return_variance else None, k_sigma)
    _check(lib().rt_denoise_var_host(int(device), w, h, C.byref(p), C.byref(pl), C.byref(v)))
    res = (out,) + ((out8,) if rgb8 else ()) + ((out_var,) if return_variance else ())
    return res if len(res) > 1 else out


def denoise_device(device, stream, w, h, *, linear_ptr, normal_ptr, albedo_ptr, z_ptr, out_ptr, object_id_ptr=None, rgb8_ptr=None,
                   sync=True, variance_ptr=None, out_variance_ptr=None, k_sigma=4.0, **params):
    """rt_denoise_device: the same on image-sized DEVICE planes (e.g. torch tensors' data_ptr()), enqueued on `stream` (an
    explicit stream's handle; None = the null stream of the device).  out_ptr may be linear_ptr (in place).
    variance_ptr: the variance-guided filter (rt_denoise_var_device); out_variance_ptr (optional, may be variance_ptr) receives
    the filtered variance."""
    pl = DenoisePlanes(rgb_linear=linear_ptr, normal=normal_ptr, albedo=albedo_ptr, z=z_ptr, object_id=object_id_ptr,
                       out_linear=out_ptr, out_rgb8=rgb8_ptr)
    p = denoise_params(**params)
    if variance_ptr is None:
        if out_variance_ptr is not None:
            raise TypeError("out_variance_ptr needs variance_ptr")
        _check(lib().rt_denoise_device(int(device), _stream_handle(stream), int(w), int(h), C.byref(p), C.byref(pl), 1 if sync else 0))
        return
    v = denoise_var(variance_ptr, out_variance_ptr, k_sigma)
    _check(lib().rt_denoise_var_device(int(device), _stream_handle(stream), int(w), int(h), C.byref(p), C.byref(pl), C.byref(v),
                                       1 if sync else 0))


_denoise = denoise       # for Scene.render_temporal, whose `denoise` argument hides the function


def temporal_params(**kw):
    """rt_temporal_default_params, then the keywords (alpha, max_history, sigma_normal, sigma_depth, gamma)"""
    return _fill_params(TemporalParams, "rt_temporal_default_params", ("alpha", "max_history", "sigma_normal", "sigma_depth", "gamma"), (), kw, "temporal")


def temporal_clip(clip=True, out_clipped=None):
    """rt_temporal_clip_default, then `clip`: True keeps the defaults, a dict overrides fields (radius, k_clip, min_count,
    clip_history).  out_clipped: the address of the optional mask plane (host or device, as the call it goes to)."""
    c = _fill_params(TemporalClip, "rt_temporal_clip_default", ("radius", "k_clip", "min_count", "clip_history"), (),
                     {} if clip is True else dict(clip), "temporal clip")
    c.out_clipped = out_clipped
    return c


def _motion_nodes(nodes, prev_nodes):
    nodes = _c(nodes, NODE)
    prev = _c(prev_nodes, NODE) if prev_nodes is not None else None
    if prev is not None and len(prev) != len(nodes):
        raise ValueError(f"prev_nodes holds {len(prev)} nodes, nodes {len(nodes)}")
    return nodes, prev


def motion(cam, prev_cam, nodes, prev_nodes, z, object_id, device=0):
    """rt_motion on host arrays: where each pixel's surface point was in the previous frame's image (rt_mi355x.h, "motion
    vectors").  nodes / prev_nodes: NODE arrays of this frame and the previous one (prev_nodes=None: nothing moved); z float32
    (H, W) and object_id int32 (H, W) of the new frame.  Returns float32 (H, W, 3): fx, fy, z_exp (z_exp <= 0: no previous
    position)."""
    nodes, prev = _motion_nodes(nodes, prev_nodes)
    z, ids = _c(z, np.float32), _c(object_id, np.int32)
    h, w = cam.height, cam.width
    assert z.shape == ids.shape == (h, w)
    out = np.empty((h, w, 3), np.float32)
    pl = MotionPlanes(z=z.ctypes.data, object_id=ids.ctypes.data, motion=out.ctypes.data)
    _check(lib().rt_motion(int(device), C.byref(cam), C.byref(prev_cam), _p(nodes), _p(prev) if prev is not None else None, len(nodes), C.byref(pl)))
    return out


def motion_device(device, stream, cam, prev_cam, nodes, prev_nodes, *, z_ptr, object_id_ptr, motion_ptr, sync=True):
    """rt_motion_device: the same on image-sized DEVICE planes, enqueued on `stream` (an explicit stream's handle; None = the
    null stream of the device).  nodes / prev_nodes stay host arrays; they are consumed before the call returns."""
    nodes, prev = _motion_nodes(nodes, prev_nodes)
    pl = MotionPlanes(z=z_ptr, object_id=object_id_ptr, motion=motion_ptr)
    _check(lib().rt_motion_device(int(device), _stream_handle(stream), C.byref(cam), C.byref(prev_cam), _p(nodes),
                                  _p(prev) if prev is not None else None, len(nodes), C.byref(pl), 1 if sync else 0))


class _Handle:
    """what the classes that own a library object share: self._h is its handle, close() (or the end of a with block, or the
    collector) hands it to the library function the subclass names in _destroy"""
    _destroy = None

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


def _copy_camera(cam):
    c = Camera()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(Camera))
    return c


def _pinhole(cam):
    """a copy of `cam` without its lens: what a frame is rendered with when a DepthOfField stage stands in for it"""
    c = _copy_camera(cam)
    c.dof = 0.0
    return c


class History(_Handle):
    """rt_history: the accumulated frames of one W x H stream on one device (the definition: rt_mi355x.h, "temporal
    accumulation").  Every accumulate blends a new frame into what the earlier ones left, reprojected from the camera of the
    previous call into `cam` (a STATIC scene) -- or, with a motion plane (motion() / motion_device()), from where that plane says
    each pixel was (moving nodes).  A context manager; close() (or the end of the with block) frees the device planes."""

    _destroy = "rt_history_destroy"

    def __init__(self, device, w, h):
        self._h = C.c_void_p()
        # Scene.render_temporal(moving=True): (camera, nodes) of the frame the history holds -- set by that method alone; any
        # other accumulate puts a frame into the history whose nodes are not known here, and forgets it
        self._moving = None
        self.device, self.width, self.height = int(device), int(w), int(h)
        _check(lib().rt_history_create(self.device, self.width, self.height, C.byref(self._h)))

    def reset(self):
        """the next frame starts from nothing"""
        _check(lib().rt_history_reset(self._h))
        self._moving = None

    @property
    def frames(self):
        """frames accumulated since the creation or the last reset()"""
        return int(lib().rt_history_frames(self._h))

    def accumulate(self, cam, linear, normal, albedo, z, object_id=None, variance=None, rgb8=False, return_history=False, motion=None,
                   clip=None, return_clipped=False, **params):
        """rt_temporal on host arrays: float32 (H, W, 3) linear / normal / albedo, float32 (H, W) z, optionally int32 (H, W)
        object_id and float32 (H, W, 3) variance.  Returns the accumulated float32 (H, W, 3) colour, followed -- as a tuple --
        by the accumulated variance (when `variance` is given), the gamma-encoded uint8 image (rgb8=True) and the per-pixel
        history length, float32 (H, W) (return_history=True).  params: temporal_params().
        motion: float32 (H, W, 3), this frame's motion plane (motion()) -- rt_temporal_motion takes the reprojection from it.
        clip: history rectification (rt_temporal_clip_host) -- True for the defaults, or a dict of radius, k_clip, min_count,
        clip_history; with or without `motion`.  return_clipped=True (needs clip) appends the mask, float32 (H, W): 0 no history,
        1 kept, 2 clipped."""
        self._moving = None
        if return_clipped and clip is None:
            raise TypeError("return_clipped needs clip")
        linear, normal, albedo = (_c(a, np.float32) for a in (linear, normal, albedo))
        h, w = self.height, self.width
        z = _c(z, np.float32)
        ids = _c(object_id, np.int32) if object_id is not None else None
        var = _c(variance, np.float32) if variance is not None else None
        assert linear.shape == normal.shape == albedo.shape == (h, w, 3) and z.shape == (h, w)
        assert (ids is None or ids.shape == (h, w)) and (var is None or var.shape == (h, w, 3))
        out = np.empty((h, w, 3), np.float32)
        out_var = np.empty((h, w, 3), np.float32) if var is not None else None
        out8 = np.empty((h, w, 3), np.uint8) if rgb8 else None
        hist = np.empty((h, w), np.float32) if return_history else None
        ptr = lambda a: a.ctypes.data if a is not None else None
        pl = TemporalPlanes(rgb_linear=ptr(linear), normal=ptr(normal), albedo=ptr(albedo), z=ptr(z), object_id=ptr(ids), variance=ptr(var),
                            out_linear=ptr(out), out_variance=ptr(out_var), out_history=ptr(hist), out_rgb8=ptr(out8))
        p = temporal_params(**params)
        mask = np.empty((h, w), np.float32) if return_clipped else None
        if motion is not None:
            motion = _c(motion, np.float32)
            assert motion.shape == (h, w, 3)
        if clip is not None:
            c = temporal_clip(clip, ptr(mask))
            _check(lib().rt_temporal_clip_host(self._h, C.byref(cam), C.byref(p), C.byref(c), C.byref(pl), ptr(motion)))
        elif motion is not None:
            _check(lib().rt_temporal_motion(self._h, C.byref(cam), C.byref(p), C.byref(pl), motion.ctypes.data))
        else:
            _check(lib().rt_temporal(self._h, C.byref(cam), C.byref(p), C.byref(pl)))
        res = (out,) + tuple(a for a in (out_var, out8, hist, mask) if a is not None)
        return res if len(res) > 1 else out

    def accumulate_device(self, stream, cam, *, linear_ptr, normal_ptr, albedo_ptr, z_ptr, out_ptr, object_id_ptr=None, variance_ptr=None,
                          out_variance_ptr=None, history_ptr=None, rgb8_ptr=None, sync=True, motion_ptr=None, clip=None, clipped_ptr=None,
                          **params):
        """rt_temporal_device: the same on image-sized DEVICE planes (e.g. torch tensors' data_ptr()), enqueued on `stream` (an
        explicit stream's handle; None = the null stream of the device).  out_ptr may be linear_ptr and out_variance_ptr may be
        variance_ptr (in place).  motion_ptr: this frame's motion plane on the device (rt_temporal_motion_device).
        clip: history rectification (rt_temporal_clip_device) -- True or a dict, as accumulate(); clipped_ptr (needs clip): a
        float32 (H, W) device plane for the mask."""
        self._moving = None
        if clipped_ptr is not None and clip is None:
            raise TypeError("clipped_ptr needs clip")
        pl = TemporalPlanes(rgb_linear=linear_ptr, normal=normal_ptr, albedo=albedo_ptr, z=z_ptr, object_id=object_id_ptr,
                            variance=variance_ptr, out_linear=out_ptr, out_variance=out_variance_ptr, out_history=history_ptr,
                            out_rgb8=rgb8_ptr)
        p = temporal_params(**params)
        if clip is not None:
            c = temporal_clip(clip, clipped_ptr)
            _check(lib().rt_temporal_clip_device(self._h, _stream_handle(stream), C.byref(cam), C.byref(p), C.byref(c), C.byref(pl),
                                                 C.c_void_p(motion_ptr) if motion_ptr is not None else None, 1 if sync else 0))
        elif motion_ptr is not None:
            _check(lib().rt_temporal_motion_device(self._h, _stream_handle(stream), C.byref(cam), C.byref(p), C.byref(pl),
                                                   C.c_void_p(motion_ptr), 1 if sync else 0))
        else:
            _check(lib().rt_temporal_device(self._h, _stream_handle(stream), C.byref(cam), C.byref(p), C.byref(pl), 1 if sync else 0))


def tonemap_params(operator="aces", **kw):
    """rt_tonemap_default_params, then the operator ("clamp", "reinhard", "aces" or an RT_TONEMAP_* number) and the keywords:
    auto_exposure, key, ev_bias, ev_min, ev_max, p_low, p_high, adapt_up, adapt_down, white, gamma; exposure_ev is another name
    for ev_bias (the exposure itself when auto_exposure is 0)."""
    op = TONEMAP_OPERATORS[operator] if isinstance(operator, str) else int(operator)
    p = _fill_params(ToneMapParams, "rt_tonemap_default_params",
                     ("auto_exposure", "key", "ev_bias", "ev_min", "ev_max", "p_low", "p_high", "adapt_up", "adapt_down", "white", "gamma"),
                     ("auto_exposure",), {("ev_bias" if k == "exposure_ev" else k): v for k, v in kw.items()}, "tone-mapping")
    p.op = op
    return p


def _tonemap_host(handle, device, linear, object_id, display, p):
    linear = _c(linear, np.float32)
    assert linear.ndim == 3 and linear.shape[2] == 3
    h, w = linear.shape[:2]
    ids = _c(object_id, np.int32) if object_id is not None else None
    assert ids is None or ids.shape == (h, w)
    out8 = np.empty((h, w, 3), np.uint8)
    disp = np.empty((h, w, 3), np.float32) if display else None
    pl = ToneMapPlanes(rgb_linear=linear.ctypes.data, object_id=ids.ctypes.data if ids is not None else None,
                       out_display=disp.ctypes.data if display else None, out_rgb8=out8.ctypes.data)
    _check(lib().rt_tonemap(handle, device, w, h, C.byref(p), C.byref(pl)))
    return (out8, disp) if display else out8


def tonemap(linear, exposure_ev=0.0, operator="aces", display=False, device=0, **params):
    """rt_tonemap without a state: the fixed exposure 2^exposure_ev, then the operator, on a float32 (H, W, 3) host array.
    Returns the gamma-encoded uint8 (H, W, 3) image -- and, display=True, the float32 display plane as a tuple's second.
    params: tonemap_params() (white, gamma)."""
    p = tonemap_params(operator, **dict(params, auto_exposure=0, ev_bias=exposure_ev))
    return _tonemap_host(None, device, linear, None, display, p)


class Exposure(_Handle):
    """rt_exposure: the exposure of one stream of frames on one device, adapted from frame to frame (the definition:
    rt_mi355x.h, "exposure and tone mapping").  Not tied to an image size.  A context manager; close() (or the end of the with
    block) frees the device block."""

    _destroy = "rt_exposure_destroy"

    def __init__(self, device=0):
        self._h = C.c_void_p()
        self.device = int(device)
        _check(lib().rt_exposure_create(self.device, C.byref(self._h)))

    def reset(self):
        """the next metered frame is the first again"""
        _check(lib().rt_exposure_reset(self._h))

    def _get(self):
        e, m, n = C.c_float(), C.c_double(), C.c_uint32()
        _check(lib().rt_exposure_get(self._h, C.byref(e), C.byref(m), C.byref(n)))
        return e.value, m.value, n.value

    @property
    def log2_exposure(self):
        """E: log2 of the scale the last METERED call applied (waits for it); a call with auto_exposure=0 leaves the state alone"""
        return self._get()[0]

    @property
    def log2_metered(self):
        """Lbar of the last frame that metered anything (waits)"""
        return self._get()[1]

    @property
    def metered_pixels(self):
        """n of the last metered call (waits)"""
        return self._get()[2]

    def histogram(self):
        """the 256-bin luminance histogram of the last metered call, uint32 (waits)"""
        out = np.zeros(256, np.uint32)
        _check(lib().rt_exposure_histogram(self._h, out.ctypes.data))
        return out

    def tonemap(self, linear, object_id=None, operator="aces", display=False, **params):
        """rt_tonemap on host arrays: float32 (H, W, 3) linear, optionally int32 (H, W) object_id (ids < 0 are not metered).
        Returns the gamma-encoded uint8 (H, W, 3) image -- and, display=True, the float32 display plane as a tuple's second.
        params: tonemap_params()."""
        return _tonemap_host(self._h, self.device, linear, object_id, display, tonemap_params(operator, **params))

    def tonemap_device(self, stream, w, h, *, linear_ptr, object_id_ptr=None, rgb8_ptr=None, display_ptr=None, sync=True, operator="aces", **params):
        """rt_tonemap_device: the same on image-sized DEVICE planes (e.g. torch tensors' data_ptr()), enqueued on `stream` (an
        explicit stream's handle; None = the null stream of the device) without a host round trip.  display_ptr may be
        linear_ptr (in place)."""
        pl = ToneMapPlanes(rgb_linear=linear_ptr, object_id=object_id_ptr, out_display=display_ptr, out_rgb8=rgb8_ptr)
        p = tonemap_params(operator, **params)
        _check(lib().rt_tonemap_device(self._h, self.device, _stream_handle(stream), int(w), int(h), C.byref(p), C.byref(pl), 1 if sync else 0))


def bloom_params(**kw):
    """rt_bloom_default_params, then the keywords: threshold, knee, intensity, spread, levels, exposure_ev"""
    return _fill_params(BloomParams, "rt_bloom_default_params", ("threshold", "knee", "intensity", "spread", "levels", "exposure_ev"), ("levels",), kw, "bloom")


def bloom_plan(w, h, levels=6):
    """rt_bloom_plan: (the levels a w x h frame gets, the level k_bloom_tail starts at or -1); needs no device"""
    used, tail = C.c_int32(), C.c_int32()
    _check(lib().rt_bloom_plan(int(w), int(h), int(levels), C.byref(used), C.byref(tail)))
    return used.value, tail.value


class Bloom(_Handle):
    """rt_bloom: the bloom stage of one w x h stream of frames on one device (the definition: rt_mi355x.h, "bloom"); it owns the
    pyramid's device memory.  A context manager; close() (or the end of the with block) frees it."""

    _destroy = "rt_bloom_destroy"

    def __init__(self, device, w, h):
        self._h = C.c_void_p()
        self.device, self.w, self.h = int(device), int(w), int(h)
        _check(lib().rt_bloom_create(self.device, self.w, self.h, C.byref(self._h)))

    def apply(self, linear, exposure=None, return_bloom=False, **params):
        """rt_bloom_host on a float32 (H, W, 3) host array: the bloomed plane -- and, return_bloom=True, the bloom plane alone as a
        tuple's second.  exposure: an Exposure on the same device whose scale the threshold is relative to (it is only read; a
        state without a metered frame, like None, means 2^exposure_ev).  params: bloom_params()."""
        linear = _c(linear, np.float32)
        assert linear.shape == (self.h, self.w, 3)
        out = np.empty_like(linear)
        only = np.empty_like(linear) if return_bloom else None
        pl = BloomPlanes(rgb_linear=linear.ctypes.data, out=out.ctypes.data, out_bloom=only.ctypes.data if return_bloom else None)
        p = bloom_params(**params)
        _check(lib().rt_bloom_host(self._h, exposure._h if exposure is not None else None, C.byref(p), C.byref(pl)))
        return (out, only) if return_bloom else out

    def apply_device(self, stream, *, linear_ptr, out_ptr, bloom_ptr=None, exposure=None, sync=False, **params):
        """rt_bloom_device: the same on image-sized DEVICE planes (e.g. torch tensors' data_ptr()), enqueued on `stream` (an
        explicit stream's handle; None = the null stream of the device) without a host round trip.  out_ptr may be linear_ptr
        (in place), or None when only bloom_ptr is wanted."""
        pl = BloomPlanes(rgb_linear=linear_ptr, out=out_ptr, out_bloom=bloom_ptr)
        p = bloom_params(**params)
        _check(lib().rt_bloom_device(self._h, exposure._h if exposure is not None else None, _stream_handle(stream), C.byref(p), C.byref(pl),
                                     1 if sync else 0))


def motion_blur_params(**kw):
    """rt_motion_blur_default_params, then the keywords: shutter, max_blur, samples, depth_extent"""
    return _fill_params(MotionBlurParams, "rt_motion_blur_default_params", ("shutter", "max_blur", "samples", "depth_extent"), ("max_blur", "samples"), kw,
                        "motion blur")


def motion_blur_tiles(w, h, max_blur=16):
    """rt_motion_blur_tiles: (TX, TY), the grid of max_blur x max_blur tiles over a w x h frame; needs no device"""
    tx, ty = C.c_int32(), C.c_int32()
    _check(lib().rt_motion_blur_tiles(int(w), int(h), int(max_blur), C.byref(tx), C.byref(ty)))
    return tx.value, ty.value


class MotionBlur(_Handle):
    """rt_motion_blur: the motion blur stage of one w x h stream of frames on one device (the definition: rt_mi355x.h, "motion
    blur"); it owns the tile planes' device memory.  A context manager; close() (or the end of the with block) frees it."""

    _destroy = "rt_motion_blur_destroy"

    def __init__(self, device, w, h):
        self._h = C.c_void_p()
        self.device, self.w, self.h = int(device), int(w), int(h)
        _check(lib().rt_motion_blur_create(self.device, self.w, self.h, C.byref(self._h)))

    def apply(self, linear, motion, z, return_tiles=False, **params):
        """rt_motion_blur_host on host arrays -- linear and motion float32 (H, W, 3), z float32 (H, W): the blurred plane, and,
        return_tiles=True, the unclamped neighbour-max vector per tile (float32 (TY, TX, 2)) as a tuple's second.
        params: motion_blur_params()."""
        linear, motion, z = _c(linear, np.float32), _c(motion, np.float32), _c(z, np.float32)
        assert linear.shape == (self.h, self.w, 3) and motion.shape == (self.h, self.w, 3) and z.shape == (self.h, self.w)
        p = motion_blur_params(**params)
        out = np.empty_like(linear)
        tiles = None
        if return_tiles:
            tx, ty = motion_blur_tiles(self.w, self.h, p.max_blur)
            tiles = np.empty((ty, tx, 2), np.float32)
        pl = MotionBlurPlanes(rgb_linear=linear.ctypes.data, motion=motion.ctypes.data, z=z.ctypes.data, out=out.ctypes.data,
                              out_tiles=tiles.ctypes.data if return_tiles else None)
        _check(lib().rt_motion_blur_host(self._h, C.byref(p), C.byref(pl)))
        return (out, tiles) if return_tiles else out

    def apply_device(self, stream, *, linear_ptr, motion_ptr, z_ptr, out_ptr, tiles_ptr=None, sync=False, **params):
        """rt_motion_blur_device: the same on image-sized DEVICE planes (e.g. torch tensors' data_ptr()), enqueued on `stream` (an
        explicit stream's handle; None = the null stream of the device) without a host round trip.  out_ptr may not be
        linear_ptr.  tiles_ptr: TX * TY * 2 floats (motion_blur_tiles)."""
        pl = MotionBlurPlanes(rgb_linear=linear_ptr, motion=motion_ptr, z=z_ptr, out=out_ptr, out_tiles=tiles_ptr)
        p = motion_blur_params(**params)
        _check(lib().rt_motion_blur_device(self._h, _stream_handle(stream), C.byref(p), C.byref(pl), 1 if sync else 0))


def dof_params(**kw):
    """rt_dof_default_params, then the keywords: max_coc, samples, depth_extent, aperture_scale, focus"""
    return _fill_params(DofParams, "rt_dof_default_params", ("max_coc", "samples", "depth_extent", "aperture_scale", "focus"), ("max_coc", "samples"), kw,
                        "depth of field")


def dof_tiles(w, h, max_coc=16):
    """rt_dof_tiles: (TX, TY), the grid of max_coc x max_coc tiles over a w x h frame; needs no device"""
    tx, ty = C.c_int32(), C.c_int32()
    _check(lib().rt_dof_tiles(int(w), int(h), int(max_coc), C.byref(tx), C.byref(ty)))
    return tx.value, ty.value


def dof_taps(samples=32):
    """rt_dof_taps: the stage's tap table, float32 (samples, 2) unit-disk offsets (ox, oy); needs no device"""
    xy = np.zeros((max(int(samples), 0), 2), np.float32)
    _check(lib().rt_dof_taps(int(samples), xy.ctypes.data))
    return xy


class DepthOfField(_Handle):
    """rt_dof: the depth-of-field stage of one w x h stream of frames on one device (the definition: rt_mi355x.h, "depth of
    field"); it owns the (c, D) plane's and the tile planes' device memory.  A context manager; close() (or the end of the with
    block) frees it."""

    _destroy = "rt_dof_destroy"

    def __init__(self, device, w, h):
        self._h = C.c_void_p()
        self.device, self.w, self.h = int(device), int(w), int(h)
        _check(lib().rt_dof_create(self.device, self.w, self.h, C.byref(self._h)))

    def apply(self, linear, z, cam, return_coc=False, return_tiles=False, **params):
        """rt_dof_host on host arrays -- linear float32 (H, W, 3), z float32 (H, W), cam the frame's Camera (its fov, focaldist,
        dof and size are used): the defocused plane, then -- return_coc=True -- the signed unclamped circle of confusion per
        pixel (float32 (H, W)) and -- return_tiles=True -- R per tile (float32 (TY, TX)) as a tuple's further members.
        params: dof_params()."""
        linear, z = _c(linear, np.float32), _c(z, np.float32)
        assert linear.shape == (self.h, self.w, 3) and z.shape == (self.h, self.w)
        p = dof_params(**params)
        out = np.empty_like(linear)
        coc = np.empty((self.h, self.w), np.float32) if return_coc else None
        tiles = None
        if return_tiles:
            tx, ty = dof_tiles(self.w, self.h, p.max_coc)
            tiles = np.empty((ty, tx), np.float32)
        pl = DofPlanes(rgb_linear=linear.ctypes.data, z=z.ctypes.data, out=out.ctypes.data, out_coc=coc.ctypes.data if return_coc else None,
                       out_tiles=tiles.ctypes.data if return_tiles else None)
        _check(lib().rt_dof_host(self._h, C.byref(cam), C.byref(p), C.byref(pl)))
        res = (out,) + ((coc,) if return_coc else ()) + ((tiles,) if return_tiles else ())
        return res if len(res) > 1 else out

    def apply_device(self, stream, cam, *, linear_ptr, z_ptr, out_ptr, coc_ptr=None, tiles_ptr=None, sync=False, **params):
        """rt_dof_device: the same on image-sized DEVICE planes (e.g. torch tensors' data_ptr()), enqueued on `stream` (an explicit
        stream's handle; None = the null stream of the device) without a host round trip.  out_ptr may not be linear_ptr.
        coc_ptr: W * H floats; tiles_ptr: TX * TY floats (dof_tiles)."""
        pl = DofPlanes(rgb_linear=linear_ptr, z=z_ptr, out=out_ptr, out_coc=coc_ptr, out_tiles=tiles_ptr)
        p = dof_params(**params)
        _check(lib().rt_dof_device(self._h, _stream_handle(stream), C.byref(cam), C.byref(p), C.byref(pl), 1 if sync else 0))


def identity_map(texture=MAP_NONE):
    m = np.zeros(1, TEXMAP)
    m["texture"] = texture
    m["tm"][0, [0, 4, 8]] = 1
    m["itm"][0, [0, 4, 8]] = 1
    return m


def photons_write_dat(path, photons_1based):
    """the reference's photonmap.dat: records [1..n] of a 1-based photon array, 24 bytes each"""
    a = _c(photons_1based, PHOTON)
    _check(lib().rt_photons_write_dat(str(path).encode(), _p(a), C.c_uint32(max(0, len(a) - 1))))


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
    _check(lib().rt_photon_balance(_p(a), C.c_uint32(len(a) - 1), _p(out)))
    return out


def photon_unreachable(photons_1based):
    """1-based indices into an UNBALANCED photon array of the photons LocatePhotons cannot reach after balancing"""
    a = _c(photons_1based, PHOTON)
    idx = np.zeros(8, np.uint32)
    n = C.c_uint32()
    _check(lib().rt_photon_unreachable(_p(a), C.c_uint32(len(a) - 1), _p(idx), 8, C.byref(n)))
    return idx[: n.value].copy()


def photon_unreachable_device(photons_1based, device=0):
    """the same on the GPU (rt_photon_unreachable_device): (sorted 1-based raw indices, exact); exact == False: a median key is not
    unique, only the host function answers"""
    ph = np.ascontiguousarray(photons_1based, PHOTON)
    n = len(ph) - 1
    idx = np.zeros(16, np.uint32)
    cnt, exact = C.c_uint32(), C.c_int32()
    _check(lib().rt_photon_unreachable_device(int(device), _p(ph), C.c_uint32(n), _p(idx), 16, C.byref(cnt), C.byref(exact)))
    return idx[:cnt.value].copy(), bool(exact.value)


class Scene:
    """Owns an rt_scene handle."""

    def __init__(self):
        self._h = C.c_void_p()
        _check(lib().rt_scene_create(C.byref(self._h)))
        self._keep = []

    def close(self):
        if self._h:
            lib().rt_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

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
        positions, which motion() follows its pixels through; an update without it makes the mesh rigid again"""
        if max_ratio is not None and rebuild:
            raise ValueError("update_mesh_vertices: rebuild=True and max_ratio exclude each other")
        v = _c(v, np.float32).reshape(-1, 3)
        vn = _c(vn, np.float32).reshape(-1, 3) if vn is not None else None
        if max_ratio is not None:
            q = MeshQuality(struct_size=C.sizeof(MeshQuality))
            _check(lib().rt_scene_update_mesh_vertices_auto_flags(self._h, int(index), _p(v), len(v), _p(vn) if vn is not None else None,
                                                                  len(vn) if vn is not None else 0, C.c_double(max_ratio),
                                                                  C.c_uint32(MESH_UPDATE_KEEP_PREVIOUS if keep_previous else 0), C.byref(q)))
            return q.as_dict()
        flags = (MESH_UPDATE_REBUILD if rebuild else 0) | (MESH_UPDATE_KEEP_PREVIOUS if keep_previous else 0)
        _check(lib().rt_scene_update_mesh_vertices_flags(self._h, int(index), _p(v), len(v), _p(vn) if vn is not None else None,
                                                         len(vn) if vn is not None else 0, C.c_uint32(flags)))

    def previous_positions(self):
        """how many meshes of the scene hold previous positions (from the scene store: no GPU)"""
        n = C.c_int32()
        _check(lib().rt_scene_previous_positions(self._h, C.byref(n)))
        return n.value

    def mesh_device_previous(self, index, device=0):
        """the previous positions of mesh `index` as they sit on `device` (lowered there first if need be): float32 (nv, 3), or
        None when the mesh holds none"""
        n = C.c_uint32()
        _check(lib().rt_scene_mesh_device_previous(self._h, int(device), int(index), None, 0, C.byref(n)))
        if n.value == 0:
            return None
        out = np.zeros((n.value, 3), np.float32)
        _check(lib().rt_scene_mesh_device_previous(self._h, int(device), int(index), _p(out), len(out), C.byref(n)))
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
        _check(lib().rt_scene_motion(self._h, int(shade_model), int(device), C.byref(cam), C.byref(prev_cam), _p(prev) if prev is not None else None,
                                     len(prev) if prev is not None else self.counts()["nodes"], C.c_float(depth_tol), C.byref(pl)))
        return out

    def motion_device(self, device, stream, cam, prev_cam, prev_nodes, *, z_ptr, object_id_ptr, motion_ptr, depth_tol=0.05, sync=True,
                      shade_model=SHADE_FIN):
        """rt_scene_motion_device: the same on image-sized DEVICE planes, enqueued on `stream` (an explicit stream's handle; None =
        the null stream of the device).  prev_nodes stays a host array; it is consumed before the call returns."""
        prev = _c(prev_nodes, NODE) if prev_nodes is not None else None
        pl = MotionPlanes(z=z_ptr, object_id=object_id_ptr, motion=motion_ptr)
        _check(lib().rt_scene_motion_device(self._h, int(shade_model), int(device), _stream_handle(stream), C.byref(cam), C.byref(prev_cam),
                                            _p(prev) if prev is not None else None, len(prev) if prev is not None else self.counts()["nodes"],
                                            C.c_float(depth_tol), C.byref(pl), 1 if sync else 0))

    def mesh_quality(self, index, device=0):
        """the SAH cost of mesh `index`'s tree as it sits on `device` (lowered there first if need be), by k_bvh_cost:
        dict(cost, built_cost, ratio, measure_ms, degenerate, rebuilt, not_on_device)"""
        q = MeshQuality(struct_size=C.sizeof(MeshQuality))
        _check(lib().rt_scene_mesh_quality(self._h, int(device), int(index), C.byref(q)))
        return q.as_dict()

    def mesh_update_ms(self, device=0):
        """the last in-place update on `device`: dict(upload, retri, refit in ms by HIP events, level_launches)"""
        t = MeshUpdateMs(struct_size=C.sizeof(MeshUpdateMs))
        _check(lib().rt_scene_mesh_update_ms(self._h, int(device), C.byref(t)))
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
        _check(lib().rt_scene_set_textures(self._h, _p(textures), len(textures), _p(texels), C.c_uint64(texels.size)))

    def set_material_maps(self, maps):
        maps = _c(maps, TEXMAP)
        assert len(maps) % 2 == 0
        _check(lib().rt_scene_set_material_maps(self._h, _p(maps), len(maps) // 2))

    def set_environment_maps(self, environment=None, background=None):
        e = _c(environment, TEXMAP).reshape(1) if environment is not None else None
        b = _c(background, TEXMAP).reshape(1) if background is not None else None
        _check(lib().rt_scene_set_environment_maps(self._h, _p(e) if e is not None else None, _p(b) if b is not None else None))

    def set_photons(self, balanced_1based):
        if balanced_1based is None or len(balanced_1based) < 2:
            _check(lib().rt_scene_set_photons(self._h, None, C.c_uint32(0)))
            return
        a = _c(balanced_1based, PHOTON)
        _check(lib().rt_scene_set_photons(self._h, _p(a), C.c_uint32(len(a) - 1)))

    def set_caustic_photons(self, balanced_1based):
        """the second map (P13's causticmap): same format as set_photons; used when params.caustic_k > 0"""
        if balanced_1based is None or len(balanced_1based) < 2:
            _check(lib().rt_scene_set_caustic_photons(self._h, None, C.c_uint32(0)))
            return
        a = _c(balanced_1based, PHOTON)
        _check(lib().rt_scene_set_caustic_photons(self._h, _p(a), C.c_uint32(len(a) - 1)))

    def generate_photons(self, max_photons=1000000, photon_bounce=8, seed=20171203, device=0, dat_path=None):
        """generatePhotonMap as a whole on the GPU (photon pass -> [dump] -> queryable structure); returns the stage times"""
        ms = SetupMs()
        _check(lib().rt_scene_generate_photons(self._h, int(device), C.c_uint32(int(max_photons)), int(photon_bounce), C.c_uint32(int(seed)),
                                               os.fsencode(dat_path) if dat_path else None, C.byref(ms)))
        return ms

    def set_render_flags(self, flags):
        """RENDER_* bits or 0 (the default); refused while a job on this scene is live"""
        _check(lib().rt_scene_set_render_flags(self._h, C.c_uint32(int(flags))))

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
        _check(lib().rt_scene_get_textures(self._h, None, 0, None, C.c_uint64(0), C.byref(ntex), C.byref(nbytes)))
        textures, texels = np.zeros(ntex.value, TEXTURE), np.zeros(nbytes.value, np.uint8)
        _check(lib().rt_scene_get_textures(self._h, _p(textures), len(textures), _p(texels), C.c_uint64(texels.size), None, None))
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
        _check(lib().rt_scene_mesh_device_read(self._h, int(device), int(index), C.byref(info), None, 0, None, 0, None, None, None))
        n = info.n_slots
        out = dict(info=info, nodes=np.zeros(info.n_nodes, DEVBVHNODE), slot_face=np.zeros(n, np.uint32),
                   tris=np.zeros((n, 12), np.float32), nrm=np.zeros((n, 9), np.float32), root_box=np.zeros(6, np.float32))
        _check(lib().rt_scene_mesh_device_read(self._h, int(device), int(index), C.byref(info), _p(out["nodes"]), len(out["nodes"]),
                                               _p(out["slot_face"]), n, _p(out["tris"]), _p(out["nrm"]), _p(out["root_box"])))
        return out

    # -- GPU work -------------------------------------------------------------------------------
    def trace_rays(self, rays, shade_model=SHADE_FIN, device=0):
        rays = _c(rays, np.float32).reshape(-1, 6)
        n = len(rays)
        out = dict(hit=np.zeros(n, np.uint8), z=np.zeros(n, np.float32), p=np.zeros((n, 3), np.float32),
                   N=np.zeros((n, 3), np.float32), node=np.zeros(n, np.int32), front=np.zeros(n, np.uint8))
        _check(lib().rt_trace_rays(self._h, int(shade_model), int(device), _p(rays), C.c_int64(n), _p(out["hit"]),
                                   _p(out["z"]), _p(out["p"]), _p(out["N"]), _p(out["node"]), _p(out["front"])))
        return out

    def estimate_irradiance(self, k, radius, pos, normal, device=0):
        pos, normal = _c(pos, np.float32).reshape(-1, 3), _c(normal, np.float32).reshape(-1, 3)
        irr, d = np.zeros_like(pos), np.zeros_like(pos)
        _check(lib().rt_estimate_irradiance(self._h, int(device), int(k), C.c_float(radius), _p(pos), _p(normal),
                                            C.c_int64(len(pos)), _p(irr), _p(d)))
        return irr, d

    def shade_rays(self, params, rays, device=0):
        rays = _c(rays, np.float32).reshape(-1, 6)
        n = len(rays)
        hit, rgb, z = np.zeros(n, np.uint8), np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
        _check(lib().rt_shade_rays(self._h, C.byref(params), int(device), _p(rays), C.c_int64(n), _p(hit), _p(rgb), _p(z)))
        return hit, rgb, z

    def photon_pass(self, max_photons, photon_bounce=8, seed=20171203, device=0):
        """generatePhotonMap on the GPU: returns (unbalanced 1-based photon array, attempts)."""
        out = np.zeros(int(max_photons) + 9, PHOTON)
        n, att = C.c_uint32(), C.c_uint64()
        _check(lib().rt_photon_pass(self._h, int(device), C.c_uint32(int(max_photons)), int(photon_bounce),
                                    C.c_uint32(int(seed)), _p(out), C.c_uint32(len(out)), C.byref(n), C.byref(att)))
        return out[: n.value + 1].copy(), att.value

    def caustic_pass(self, max_diffuse_hits, photon_bounce=5, seed=20171203, device=0):
        """P13's caustic loop on the GPU: returns (unbalanced 1-based photon array, attempts)."""
        out = np.zeros(int(max_diffuse_hits) + 9, PHOTON)
        n, att = C.c_uint32(), C.c_uint64()
        _check(lib().rt_caustic_pass(self._h, int(device), C.c_uint32(int(max_diffuse_hits)), int(photon_bounce),
                                     C.c_uint32(int(seed)), _p(out), C.c_uint32(len(out)), C.byref(n), C.byref(att)))
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

    def render_tiles_outputs_device(self, cam, params, tiles, device, rgb_ptr, z_ptr, cnt_ptr, stream=None, sync=True,
                                    want_stats=True, linear_ptr=None, normal_ptr=None, albedo_ptr=None, alpha_ptr=None,
                                    object_id_ptr=None, variance_ptr=None):
        """render_tiles_device through rt_render_tiles_outputs_device: every *_ptr that is not None names an image-sized
        DEVICE plane to fill (float32 x 3 for linear / normal / albedo, float32 for alpha, int32 for object_id).
        variance_ptr (float32 x 3): through rt_render_tiles_outputs_var_device."""
        st = Stats()
        o = Outputs(rgb8=rgb_ptr, z=z_ptr, count=cnt_ptr, rgb_linear=linear_ptr, normal=normal_ptr, albedo=albedo_ptr,
                    alpha=alpha_ptr, object_id=object_id_ptr)
        if variance_ptr is not None:
            _check(lib().rt_render_tiles_outputs_var_device(self._h, C.byref(cam), C.byref(params), C.byref(tiles), int(device),
                                                            _stream_handle(stream), C.byref(o), C.c_void_p(variance_ptr),
                                                            1 if sync else 0, C.byref(st) if want_stats else None))
            return st
        _check(lib().rt_render_tiles_outputs_device(self._h, C.byref(cam), C.byref(params), C.byref(tiles), int(device),
                                                    _stream_handle(stream), C.byref(o), 1 if sync else 0,
                                                    C.byref(st) if want_stats else None))
        return st

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
        if planes is not None:
            o = Outputs(rgb8=rgb.ctypes.data, z=z.ctypes.data, count=cnt.ctypes.data,
                        **{OUTPUT_PLANES[name][0]: a.ctypes.data for name, a in planes.items() if name != "variance"})
            if "variance" in planes:
                _check(lib().rt_render_begin_outputs_var(self._h, C.byref(cam), C.byref(params), C.byref(tiles), int(device),
                                                         C.byref(o), planes["variance"].ctypes.data, C.byref(job)))
            else:
                _check(lib().rt_render_begin_outputs(self._h, C.byref(cam), C.byref(params), C.byref(tiles), int(device),
                                                     C.byref(o), C.byref(job)))
        elif linear is None:
            _check(lib().rt_render_begin(self._h, C.byref(cam), C.byref(params), C.byref(tiles), int(device),
                                         _p(rgb), _p(z), _p(cnt), C.byref(job)))
        else:
            _check(lib().rt_render_begin_linear(self._h, C.byref(cam), C.byref(params), C.byref(tiles), int(device),
                                                _p(rgb), _p(z), _p(cnt), _p(linear), C.byref(job)))
        try:
            _check(lib().rt_render_wait(job))
            st = Stats()
            _check(lib().rt_job_stats(job, C.byref(st)))
            progress = lib().rt_render_progress(job)
        finally:
            lib().rt_job_destroy(job)
        return rgb, z, cnt, st, progress

    def render_tiles_packed_device(self, cam, params, tiles, device, packed_ptr, packed_bytes, stream=None, sync=True,
                                   want_stats=True, linear=False):
        """This call's tiles as packed 8-byte pixel records (the all-gather contribution of a rank), see the header.
        linear=True: 24-byte records that also hold the linear plane (tiles_packed_size(..., linear=True) bytes)."""
        st = Stats()
        handle = _stream_handle(stream)
        fn = lib().rt_render_tiles_packed_linear_device if linear else lib().rt_render_tiles_packed_device
        _check(fn(self._h, C.byref(cam), C.byref(params), C.byref(tiles), int(device), handle,
                  C.c_void_p(packed_ptr), C.c_uint64(int(packed_bytes)), 1 if sync else 0,
                  C.byref(st) if want_stats else None))
        return st

    def render_tiles_packed_outputs_device(self, cam, params, tiles, device, packed_ptr, packed_bytes, stream=None, sync=True,
                                           want_stats=True, planes=()):
        """render_tiles_packed_device with the planes named in `planes` (those of render_outputs) as sections behind the records:
        one rank's contribution in the packed planes format, tiles_packed_planes_size(..., planes) bytes.  Slots of no pixel are
        zeroed by the call."""
        st = Stats()
        _check(lib().rt_render_tiles_packed_outputs_device(self._h, C.byref(cam), C.byref(params), C.byref(tiles), int(device),
                                                           _stream_handle(stream), C.c_void_p(packed_ptr), C.c_uint64(int(packed_bytes)),
                                                           plane_mask(planes), 1 if sync else 0, C.byref(st) if want_stats else None))
        return st

    def render_counters(self, device=0, reset=False):
        """the device-side work counters accumulated since they were last cleared (rt_render_counters); waits for pending renders"""
        st = Stats()
        _check(lib().rt_render_counters(self._h, int(device), 1 if reset else 0, C.byref(st)))
        return st

    def render_check(self, device=0):
        """Collect the verdict of the asynchronous renders issued so far (raises on dropped rays)."""
        _check(lib().rt_render_check(self._h, int(device)))

    def render_tiles_device(self, cam, params, tiles, device, rgb_ptr, z_ptr, cnt_ptr, stream=None, sync=True,
                            want_stats=True, linear_ptr=None):
        """Render this call's tiles into DEVICE buffers (e.g. torch tensors' data_ptr()).
        stream: None = the library's own stream; otherwise the handle of an EXPLICIT hipStream_t.  0 -- what torch
        reports for its legacy default stream -- is refused: through this argument NULL means "the library's
        stream", so work on the default stream would silently not be ordered with the render; run the caller's
        side under a torch.cuda.Stream and pass its handle (raytracing_folder_amd.dist does).
        linear_ptr: also the linear plane (float32 (H, W, 3) on the device), through rt_render_tiles_linear_device."""
        st = Stats()
        handle = _stream_handle(stream)
        if linear_ptr is None:
            _check(lib().rt_render_tiles_device(self._h, C.byref(cam), C.byref(params), C.byref(tiles), int(device),
                                                handle, C.c_void_p(rgb_ptr),
                                                C.c_void_p(z_ptr), C.c_void_p(cnt_ptr), 1 if sync else 0,
                                                C.byref(st) if want_stats else None))
        else:
            _check(lib().rt_render_tiles_linear_device(self._h, C.byref(cam), C.byref(params), C.byref(tiles), int(device),
                                                       handle, C.c_void_p(rgb_ptr), C.c_void_p(z_ptr), C.c_void_p(cnt_ptr),
                                                       C.c_void_p(linear_ptr), 1 if sync else 0,
                                                       C.byref(st) if want_stats else None))
        return st
