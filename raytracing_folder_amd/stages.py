"""The image-space stages of librt_mi355x.so (csrc/rt_post.cpp) on the ABI of abi.py: denoise, motion vectors, temporal
accumulation, exposure and tone mapping, bloom, motion blur, depth of field.  Reached through capi.py, which imports all of it."""
from .abi import *  # noqa: F401,F403
from .abi import _Handle, _c, _check, _p, _stream_handle


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
        _check(lib().rt_denoise(device, w, h, C.byref(p), C.byref(pl)))
        return (out, out8) if rgb8 else out
    variance = _c(variance, np.float32)
    assert variance.shape == (h, w, 3)
    out_var = np.empty((h, w, 3), np.float32) if return_variance else None
    v = denoise_var(variance.ctypes.data, out_var.ctypes.data if return_variance else None, k_sigma)
    _check(lib().rt_denoise_var_host(device, w, h, C.byref(p), C.byref(pl), C.byref(v)))
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
        _check(lib().rt_denoise_device(device, _stream_handle(stream), int(w), int(h), C.byref(p), C.byref(pl), 1 if sync else 0))
        return
    v = denoise_var(variance_ptr, out_variance_ptr, k_sigma)
    _check(lib().rt_denoise_var_device(device, _stream_handle(stream), int(w), int(h), C.byref(p), C.byref(pl), C.byref(v), 1 if sync else 0))


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
    _check(lib().rt_motion(device, C.byref(cam), C.byref(prev_cam), _p(nodes), _p(prev), len(nodes), C.byref(pl)))
    return out


def motion_device(device, stream, cam, prev_cam, nodes, prev_nodes, *, z_ptr, object_id_ptr, motion_ptr, sync=True):
    """rt_motion_device: the same on image-sized DEVICE planes, enqueued on `stream` (an explicit stream's handle; None = the
    null stream of the device).  nodes / prev_nodes stay host arrays; they are consumed before the call returns."""
    nodes, prev = _motion_nodes(nodes, prev_nodes)
    pl = MotionPlanes(z=z_ptr, object_id=object_id_ptr, motion=motion_ptr)
    _check(lib().rt_motion_device(device, _stream_handle(stream), C.byref(cam), C.byref(prev_cam), _p(nodes), _p(prev), len(nodes),
                                  C.byref(pl), 1 if sync else 0))


class History(_Handle):
    """rt_history: the accumulated frames of one W x H stream on one device (the definition: rt_mi355x.h, "temporal
    accumulation").  Every accumulate blends a new frame into what the earlier ones left, reprojected from the camera of the
    previous call into `cam` (a STATIC scene) -- or, with a motion plane (motion() / motion_device()), from where that plane says
    each pixel was (moving nodes).  A context manager; close() (or the end of the with block) frees the device planes."""

    _create, _destroy, _size = "rt_history_create", "rt_history_destroy", ("width", "height")
    # Scene.render_temporal(moving=True): (camera, nodes) of the frame the history holds -- set by that method alone; any
    # other accumulate puts a frame into the history whose nodes are not known here, and forgets it
    _moving = None

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
        c = temporal_clip(clip, clipped_ptr) if clip is not None else None
        head, sync = (self._h, _stream_handle(stream), C.byref(cam), C.byref(p)), 1 if sync else 0
        if clip is not None:
            _check(lib().rt_temporal_clip_device(*head, C.byref(c), C.byref(pl), motion_ptr, sync))
        elif motion_ptr is not None:
            _check(lib().rt_temporal_motion_device(*head, C.byref(pl), motion_ptr, sync))
        else:
            _check(lib().rt_temporal_device(*head, C.byref(pl), sync))


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

    _create, _destroy = "rt_exposure_create", "rt_exposure_destroy"

    def __init__(self, device=0):
        super().__init__(device)

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

    _create, _destroy, _size = "rt_bloom_create", "rt_bloom_destroy", ("w", "h")

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

    _create, _destroy, _size = "rt_motion_blur_create", "rt_motion_blur_destroy", ("w", "h")

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

    _create, _destroy, _size = "rt_dof_create", "rt_dof_destroy", ("w", "h")

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
