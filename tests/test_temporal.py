"""Temporal accumulation with camera reprojection (rt_history_*, rt_temporal, rt_temporal_device, k_temporal; capi.History,
capi.temporal_params, Scene.render_temporal; rt::RenderImage::EnableTemporal / AccumulateTemporal).  The reference has no
counterpart, so the yardstick is `ref_temporal` below: a float64 numpy transcription of the header's definition ("temporal
accumulation") that carries its own history from frame to frame, itself checked on the CPU through properties that do not depend
on the transcription (a repeated camera, the closed form of the blend weights, an affine light under a moved camera).  Its input
is `frame`: an analytic scene -- a wall, a square in front of it, a strip where nothing is hit -- seen through any rt_camera."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from raytracing_folder_amd import capi
from tests import scenes
from tests.stage_support import BIG, F, assert_driver_usage, build_driver, gi_params as _gi_params, valid as _valid

BG = (0.25, 0.5, 0.75)
MARGIN = 1e-3                   # a pixel closer than this to a decision of the definition is left out of GPU comparisons ...
MAX_LEFT_OUT = 0.02             # ... and at most this share of a frame's valid pixels may be
SIZES = ((37, 23), (1, 1), (3, 2), (5, 40))


# ---- cameras ----------------------------------------------------------------------------------------------------
def make_cam(w, h, pos=(0.0, 0.0, 10.0), yaw=0.0):
    """fov 40, looking down -z from `pos`, turned by `yaw` degrees about y"""
    cam = capi.Camera()
    t = math.radians(yaw)
    cam.pos[:], cam.dir[:], cam.up[:] = pos, (-math.sin(t), 0.0, -math.cos(t)), (0.0, 1.0, 0.0)
    cam.fov, cam.focaldist, cam.dof, cam.width, cam.height = 40.0, 1.0, 0.0, w, h
    return cam


def cam_a(w, h):
    return make_cam(w, h)


def cam_b(w, h):
    return make_cam(w, h, pos=(0.6, -0.25, 10.4))              # A translated by (0.6, -0.25, 0.4)


def cam_c(w, h):
    return make_cam(w, h, yaw=3.0)


def cam_setup(cam):
    """camera_setup's quantities, computed in float32 as the library computes them (tan in double), held as float64"""
    W, H = cam.width, cam.height
    l = F(cam.focaldist)
    hh = F(2.0 * float(l) * math.tan(float(F(cam.fov)) / 2 * (math.pi / 180)))
    ww = F(F(hh * F(W)) / F(H))
    u, v = F(ww / F(W)), F(-hh / F(H))
    b = np.array([F(-ww / F(2)) + F(u / F(2)), F(hh / F(2)) + F(v / F(2)), -l], F)
    up = np.array(list(cam.up), F)
    z_new = -np.array(list(cam.dir), F)
    cross = lambda p, q: np.array([F(p[1] * q[2]) - F(p[2] * q[1]), F(p[2] * q[0]) - F(p[0] * q[2]), F(p[0] * q[1]) - F(p[1] * q[0])], F)
    x_new = cross(up, z_new)
    norm = lambda p: (p / np.sqrt(F(F(F(p[0] * p[0]) + F(p[1] * p[1])) + F(p[2] * p[2])))).astype(F)
    M = np.stack([norm(x_new), norm(up), norm(z_new)], axis=1).astype(np.float64)       # columns x_new, up, z_new
    return dict(pos=np.array(list(cam.pos), np.float64), M=M, b=b.astype(np.float64), u=float(u), v=float(v), W=W, H=H)


def pixel_rays(cs):
    """the representative ray of every pixel: unit directions (H, W, 3), float64"""
    Y, X = np.mgrid[0:cs["H"], 0:cs["W"]]
    s = np.stack([cs["b"][0] + (X + 0.5) * cs["u"], cs["b"][1] + (Y + 0.5) * cs["v"], np.full(X.shape, cs["b"][2])], -1)
    d = s @ cs["M"].T
    return d / np.sqrt((d * d).sum(-1))[..., None]


# ---- the synthetic frame ----------------------------------------------------------------------------------------
def light_smooth(P):
    return 0.6 + 0.3 * np.sin(P[..., 0]) * np.cos(0.7 * P[..., 1])


def light_affine(P):
    return 0.5 + 0.05 * P[..., 0] + 0.03 * P[..., 1] + 0.02 * P[..., 2]


WALL_EDGE, SQUARE_Z, SQUARE_HALF = 4.0, 4.0, 0.8
SQUARE_NORMAL = (0.6, 0.0, 0.8)


def frame(cam, seed, noise, light=light_smooth, dtype=np.float32):
    """What `cam` sees of a static world, computed exactly from each pixel's representative ray: a wall in the plane z = 0 for
    x < 4 (id 3, normal +z, albedo in two vertical halves split at x = 0, a patch of zero albedo about 3 x 3 pixels large at
    37 x 23), in front of it at z = 4 an axis-aligned square of half-size 0.8 (id 4, another normal), and beyond the wall's
    edge nothing (id -1, z = 1e30, the background colour).  z is the Euclidean distance along the ray.  colour = clean x
    (1 + noise N(0, 1)) with clean = albedo x light(P) (the zero-albedo patch: light(P)); variance = (noise clean)^2.
    Returns (planes dict, clean colour)."""
    cs = cam_setup(cam)
    d, o = pixel_rays(cs), cs["pos"]
    down = d[..., 2] < 0
    dz = np.where(down, d[..., 2], -1.0)
    t_sq, t_wall = (SQUARE_Z - o[2]) / dz, (0.0 - o[2]) / dz
    P_sq, P_wall = o + t_sq[..., None] * d, o + t_wall[..., None] * d
    hit_sq = down & (t_sq > 0) & (np.abs(P_sq[..., 0]) <= SQUARE_HALF) & (np.abs(P_sq[..., 1]) <= SQUARE_HALF)
    hit_wall = down & (t_wall > 0) & (P_wall[..., 0] < WALL_EDGE) & ~hit_sq
    hit = hit_sq | hit_wall
    P = np.where(hit_sq[..., None], P_sq, P_wall)
    ids = np.where(hit_sq, 4, np.where(hit_wall, 3, -1)).astype(np.int32)
    z = np.where(hit_sq, t_sq, np.where(hit_wall, t_wall, float(BIG)))
    normal = np.where(hit_sq[..., None], SQUARE_NORMAL, np.where(hit_wall[..., None], (0.0, 0.0, 1.0), (0.0, 0.0, 0.0)))
    albedo = np.where((P[..., 0] < 0)[..., None], (0.8, 0.5, 0.3), (0.2, 0.6, 0.9))
    patch = hit_wall & (P[..., 0] >= -3.0) & (P[..., 0] <= -2.05) & (P[..., 1] >= 1.0) & (P[..., 1] <= 1.95)
    albedo = np.where(patch[..., None], 0.0, albedo)
    albedo = np.where(hit_sq[..., None], 0.7, albedo)
    albedo = np.where(hit[..., None], albedo, 0.0)
    clean = np.where(albedo > 1e-3, albedo, 1.0) * light(P)[..., None]
    clean = np.where(hit[..., None], clean, BG)
    rng = np.random.default_rng(seed)
    lin = np.where(hit[..., None], clean * (1 + noise * rng.normal(0, 1, clean.shape)), clean)
    var = np.where(hit[..., None], (noise * clean) ** 2, 0.0)
    pl = dict(linear=lin.astype(dtype), normal=normal.astype(dtype), albedo=albedo.astype(dtype), z=z.astype(dtype), object_id=ids,
              variance=var.astype(dtype))
    return pl, clean.astype(dtype)


# ---- the reference ----------------------------------------------------------------------------------------------
def ref_temporal(hist, cam, pl, with_ids=True, with_var=True, alpha=0.2, max_history=32, sigma_normal=0.3, sigma_depth=0.05):
    """float64 transcription of the definition.  `hist` is the reference's own history (an empty dict = no frame yet); it is
    updated in place.  The parameters are taken as the float32 values the ABI carries.  Returns a dict: linear, variance,
    history (the three outputs), part (the pixels that take part), has (those with a history), weight (their W), margin (each pixel's smallest
    margin to a decision: q.z to 0 and W to 0.01 absolute, fx / fy in pixels to -1 and to the image's size -- the positions
    beyond which no tap lies inside the image; where a single tap enters or leaves the image, at 0 and size - 1, its weight
    is 0 and nothing is decided --, the depth and normal tests relative to their thresholds), left_out (margin < 1e-3, or a
    tap with weight reads a pixel that was itself left out in the frame before: the GPU's history may differ there), and
    s_linear, s_variance, s_history: the spread (max - min) of the accepted taps' stored values, remodulated."""
    al, sn, sd = (float(F(v)) for v in (alpha, sigma_normal, sigma_depth))
    cs = cam_setup(cam)
    H, W = cs["H"], cs["W"]
    lin, n64, z64 = (pl[k].astype(np.float64) for k in ("linear", "normal", "z"))
    ids = pl["object_id"] if with_ids else None
    valid = (ids >= 0) if with_ids else (pl["z"] < BIG)
    a = np.where(pl["albedo"] > F(1e-3), pl["albedo"], 1).astype(np.float64)
    with np.errstate(all="ignore"):
        d = lin / a
        part = valid & np.isfinite(d).all(-1)
        v64 = pl["variance"].astype(np.float64) if with_var else np.zeros_like(lin)
        u = np.where(np.isfinite(v64) & (v64 > 0), v64, 0.0) / a ** 2
        idp = ids if with_ids else np.zeros((H, W), np.int32)
        margin = np.full((H, W), np.inf)
        tainted = np.zeros((H, W), bool)
        Wsum, nsum = np.zeros((H, W)), np.zeros((H, W))
        dsum, usum = np.zeros((H, W, 3)), np.zeros((H, W, 3))
        lo = dict(d=np.full((H, W, 3), np.inf), u=np.full((H, W, 3), np.inf), N=np.full((H, W), np.inf))
        hi = {k: -v for k, v in lo.items()}
        geom = np.zeros((H, W), bool)
        if hist:
            old = hist["cam"]
            P = cs["pos"] + np.where(part, z64, 1.0)[..., None] * pixel_rays(cs)
            e = P - old["pos"]
            q = e @ old["M"]                                    # (x_new', up', z_new') . e
            geom = q[..., 2] < 0
            margin = np.minimum(margin, np.abs(q[..., 2]))
            t = old["b"][2] / np.where(geom, q[..., 2], -1.0)
            fx, fy = (q[..., 0] * t - old["b"][0]) / old["u"] - 0.5, (q[..., 1] * t - old["b"][1]) / old["v"] - 0.5
            zexp = np.sqrt((e * e).sum(-1))
            for f, size in ((fx, W), (fy, H)):
                margin = np.minimum(margin, np.where(geom, np.minimum(np.abs(f + 1), np.abs(f - size)), np.inf))
            x0, y0 = np.floor(fx), np.floor(fy)
            tx, ty = fx - x0, fy - y0
            for k in range(4):                                  # (0,0), (1,0), (0,1), (1,1)
                i, j = k & 1, k >> 1
                qx, qy = x0 + i, y0 + j
                inside = geom & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                qx, qy = np.clip(qx, 0, W - 1).astype(int), np.clip(qy, 0, H - 1).astype(int)
                w = (tx if i else 1 - tx) * (ty if j else 1 - ty)
                reach = inside & (hist["N"][qy, qx] > 0) & ((hist["id"][qy, qx] == idp) if with_ids else True)
                dn2 = ((hist["n"][qy, qx] - n64) ** 2).sum(-1)
                dzq, thr = np.abs(hist["z"][qy, qx] - zexp), sd * np.maximum(hist["z"][qy, qx], zexp)
                margin = np.minimum(margin, np.where(reach, np.abs(dn2 - sn * sn) / (sn * sn), np.inf))
                margin = np.minimum(margin, np.where(reach, np.abs(dzq - thr) / thr, np.inf))
                acc = reach & (dn2 <= sn * sn) & (dzq <= thr)
                tainted |= inside & (w > 0) & hist["left_out"][qy, qx]
                wa = np.where(acc, w, 0.0)
                Wsum += wa
                nsum += wa * hist["N"][qy, qx]
                dsum += wa[..., None] * np.where(acc[..., None], hist["d"][qy, qx], 0.0)
                usum += wa[..., None] * np.where(acc[..., None], hist["u"][qy, qx], 0.0)
                for key in ("d", "u", "N"):
                    m = acc if key == "N" else acc[..., None]
                    lo[key] = np.minimum(lo[key], np.where(m, hist[key][qy, qx], np.inf))
                    hi[key] = np.maximum(hi[key], np.where(m, hist[key][qy, qx], -np.inf))
            margin = np.minimum(margin, np.where(geom, np.abs(Wsum - 0.01), np.inf))
        has = part & geom & (Wsum >= 0.01)
        safe = np.where(has, Wsum, 1.0)
        N = np.where(has, np.minimum(nsum / safe + 1, float(max_history)), 1.0)
        beta = np.maximum(al, 1.0 / N)[..., None]
        d2 = np.where(has[..., None], (1 - beta) * dsum / safe[..., None] + beta * d, d)
        u2 = np.where(has[..., None], (1 - beta) ** 2 * usum / safe[..., None] + beta ** 2 * u, u)
        N = np.where(part, N, 0.0)
        left_out = part & ((margin < MARGIN) | tainted)
        spread = {k: np.where(has if k == "N" else has[..., None], hi[k] - lo[k], 0.0) for k in lo}
        hist.clear()
        hist.update(cam=cs, d=d2, u=u2, N=N, z=z64, n=n64, id=np.where(part, idp, -1), left_out=left_out)
        return dict(linear=np.where(part[..., None], d2 * a, lin), variance=np.where(part[..., None], u2 * a ** 2, v64), history=N,
                    part=part, has=has, weight=np.where(has, Wsum, 0.0), margin=margin, left_out=left_out, s_linear=spread["d"] * a, s_variance=spread["u"] * a ** 2,
                    s_history=spread["N"])


def delta_px(cam_old, cam_new, z_min):
    """A bound on the float32 error of the reprojected position, |error of fx| + |error of fy| in pixels, from the operation
    chain of steps 2-3 of the definition as k_temporal runs it (every operation rounds once, relative error at most 2^-24):
      s = b + (x + 0.5) u                  2   (x + 0.5 is exact)
      M s, one component                   5   (three products, two sums)
      normalize: |r|^2, sqrt, 1 / x, r * x 8
      P = pos + z r                        2
      e = P - pos'                         1
      q = rows . e, one component          5
      -l' / q.z, q * that                  2
      (s' - b') / u' - 0.5                 3
    28 in all, and 4 more for the camera quantities themselves (cam_setup above repeats the library's float32 set-up, up to
    the rounding of its normalisations): 32.  A relative error of the position is worth at most the position's magnitude in
    pixels, W for fx and H for fy; the errors made before the subtraction P - pos' are relative to |pos| + z and |pos'|, but
    count relative to |e| ~ z afterwards, hence the factor 1 + (|pos| + |pos'|) / z_min.
      delta_px = 32 * 2^-24 * (W + H) * (1 + (|pos| + |pos'|) / z_min)
    which is 5e-4 pixels for cameras A and B at 37 x 23 (z_min = 6)."""
    norm = lambda c: math.sqrt(sum(float(x) ** 2 for x in c.pos))
    return 32 * 2.0 ** -24 * (cam_new.width + cam_new.height) * (1 + (norm(cam_old) + norm(cam_new)) / z_min)


def _planes_for(pl, with_ids, with_var):
    return dict(object_id=pl["object_id"] if with_ids else None, variance=pl["variance"] if with_var else None)


def _sequence(cams, noise, with_ids=True, with_var=True, light=light_smooth, dtype=np.float32, seed=100, **params):
    """the reference over a sequence of cameras with fresh noise per frame: [(cam, planes, clean, result)]"""
    hist, out = {}, []
    for k, cam in enumerate(cams):
        pl, clean = frame(cam, seed + k, noise, light, dtype)
        out.append((cam, pl, clean, ref_temporal(hist, cam, pl, with_ids, with_var, **params)))
    return out


# ---- CPU: the ABI -----------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("rt_history_create", "rt_history_reset", "rt_history_destroy", "rt_history_frames", "rt_temporal_default_params",
               "rt_temporal_device", "rt_temporal")


def test_new_symbols_struct_layout_and_defaults():
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert L.rt_abi_version() == 4
    assert [f[0] for f in capi.TemporalParams._fields_] == ["struct_size", "alpha", "max_history", "sigma_normal", "sigma_depth", "gamma"]
    assert [f[0] for f in capi.TemporalPlanes._fields_] == ["struct_size", "rgb_linear", "normal", "albedo", "z", "object_id", "variance",
                                                            "out_linear", "out_variance", "out_history", "out_rgb8"]
    assert C.sizeof(capi.TemporalParams) == 24 and C.sizeof(capi.TemporalPlanes) == 88
    p = capi.TemporalParams()
    L.rt_temporal_default_params(C.byref(p))
    assert (p.struct_size, p.alpha, p.max_history, p.sigma_normal, p.sigma_depth, p.gamma) == (24, F(0.2), 32, F(0.3), F(0.05), F(2.2))
    L.rt_temporal_default_params(None)                          # ignored
    q = capi.temporal_params(alpha=0.5, max_history=8)
    assert q.alpha == 0.5 and q.max_history == 8 and q.sigma_normal == F(0.3)
    with pytest.raises(TypeError):
        capi.temporal_params(levels=3)
    # the existing structs did not grow
    assert C.sizeof(capi.Outputs) == 72 and C.sizeof(capi.DenoiseParams) == 24 and C.sizeof(capi.DenoisePlanes) == 64 and C.sizeof(capi.DenoiseVar) == 32
    assert L.rt_history_frames(None) == 0
    L.rt_history_destroy(None)                                  # ignored


def _arg_cases():
    """(what the last error must name, params, planes) for every argument check that needs no history"""
    buf = np.zeros(8 * 8 * 3, np.float32)
    ptr = buf.ctypes.data
    full = lambda **kw: capi.TemporalPlanes(**{**dict(rgb_linear=ptr, normal=ptr, albedo=ptr, z=ptr, object_id=ptr, variance=ptr, out_linear=ptr,
                                                      out_variance=ptr, out_history=ptr, out_rgb8=ptr), **kw})
    cases = []
    for bad in (0, 23, 32):
        p = capi.temporal_params()
        p.struct_size = bad
        cases.append((b"struct_size", p, full()))
    pl = full()
    pl.struct_size += 8
    cases.append((b"struct_size", capi.temporal_params(), pl))
    for bad in (0.0, -0.1, 1.5, float("nan"), float("inf")):
        cases.append((b"alpha", capi.temporal_params(alpha=bad), full()))
    for bad in (0, -1, 65536):
        cases.append((b"max_history", capi.temporal_params(max_history=bad), full()))
    for name in ("sigma_normal", "sigma_depth", "gamma"):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            cases.append((b"positive and finite", capi.temporal_params(**{name: bad}), full()))
    for name in ("rgb_linear", "normal", "albedo", "z", "out_linear"):
        cases.append((b"required", capi.temporal_params(), full(**{name: None})))
    cases.append((b"out_variance needs", capi.temporal_params(), full(variance=None)))
    return buf, cases, full


def test_argument_checks_come_before_any_gpu_call():
    """without a history (a machine without a GPU cannot make one) every check but the camera's size is still reached: the
    NULL history is refused last"""
    L = capi.lib()
    cam = cam_a(8, 8)
    buf, cases, full = _arg_cases()
    for what, p, pl in cases:
        for st in (L.rt_temporal(None, C.byref(cam), C.byref(p), C.byref(pl)), L.rt_temporal_device(None, None, C.byref(cam), C.byref(p), C.byref(pl), 1)):
            assert st == -1 and what in L.rt_last_error(), (what, L.rt_last_error())
    p, pl = capi.temporal_params(), full()
    for args in ((None, C.byref(p), C.byref(pl)), (C.byref(cam), None, C.byref(pl)), (C.byref(cam), C.byref(p), None)):
        assert L.rt_temporal(None, *args) == -1 and L.rt_temporal_device(None, None, *args, 1) == -1
    assert L.rt_temporal(None, C.byref(cam), C.byref(p), C.byref(pl)) == -1 and b"history is NULL" in L.rt_last_error()
    assert L.rt_temporal_device(None, None, C.byref(cam), C.byref(p), C.byref(pl), 1) == -1 and b"history is NULL" in L.rt_last_error()
    assert L.rt_history_reset(None) == -1
    h = C.c_void_p()
    assert L.rt_history_create(0, 0, 8, C.byref(h)) == -1 and L.rt_history_create(0, 8, -1, C.byref(h)) == -1 and not h
    assert L.rt_history_create(0, 8, 8, None) == -1
    if capi.device_count() == 0:
        assert L.rt_history_create(0, 8, 8, C.byref(h)) == -3 and not h
        with pytest.raises(capi.RtError) as e:
            capi.History(0, 8, 8)
        assert e.value.status == -3


def test_shim_driver_builds_against_the_header(tmp_path):
    assert_driver_usage(build_driver(tmp_path, "shim_temporal_driver"))


# ---- CPU: the reference and the synthetic frame -----------------------------------------------------------------
def test_frame_holds_what_the_tests_rely_on():
    pl, clean = frame(cam_a(37, 23), 0, 0.3)
    ids = pl["object_id"]
    assert (ids == 3).sum() > 500 and 50 < (ids == 4).sum() < 150 and 50 < (ids == -1).sum() < 250
    assert (pl["z"][ids == -1] == BIG).all() and np.allclose(pl["z"][ids == 4].min(), 6.0, atol=0.05) and pl["z"][ids == 3].min() >= 10
    patch = (ids == 3) & (pl["albedo"] == 0).all(-1)
    assert 6 <= patch.sum() <= 12
    assert len(np.unique(pl["albedo"][(ids == 3) & ~patch], axis=0)) == 2
    assert (pl["variance"][ids >= 0] > 0).all() and (pl["linear"][ids == -1] == F(BG)).all()


def test_reference_with_a_repeated_camera_and_no_noise_returns_the_input():
    cams = [cam_a(37, 23)] * 5
    for with_ids in (True, False):
        for k, (cam, pl, clean, r) in enumerate(_sequence(cams, 0.0, with_ids, max_history=3)):
            part = _valid(pl, with_ids)
            assert (r["part"] == part).all() and (r["has"] == (part & (k > 0))).all()
            assert np.abs(r["linear"] - pl["linear"])[part].max() < 1e-12
            assert (r["history"][part] == min(k + 1, 3)).all() and (r["history"][~part] == 0).all()
            assert (r["linear"][~part] == pl["linear"][~part]).all() and not r["left_out"].any()


def test_reference_error_variance_follows_the_closed_form_of_the_weights():
    """beta_k = max(0.2, 1 / k): the plain mean for k <= 5 (variance factor 1 / k), then v' = 0.64 v + 0.04 per frame -- with
    the float32 that 0.2 is in the ABI, which the 1e-12 of the variance check sees"""
    noise, alpha = 0.3, float(F(0.2))
    seq = _sequence([cam_a(37, 23)] * 8, noise, dtype=np.float64)
    factor = 0.0
    for k, (cam, pl, clean, r) in enumerate(seq, 1):
        beta = max(alpha, 1.0 / k)
        factor = (1 - beta) ** 2 * factor + beta ** 2
        if k <= 5:
            assert abs(factor - 1.0 / k) < 1e-15
        else:
            assert abs(factor - (0.64 * prev_factor + 0.04)) < 1e-8
        prev_factor = factor
        wall = pl["object_id"] == 3
        rel = ((r["linear"] - clean) / (noise * clean))[wall]    # unit variance per frame and channel; (clean = d_clean a)
        n = rel.size
        # the sample variance of n independent unit normals scaled by `factor`: standard error factor * sqrt(2 / n); five of them
        assert abs(rel.var() - factor) < 5 * factor * math.sqrt(2.0 / n), (k, rel.var(), factor)
        want_var = (noise * clean) ** 2 * factor
        assert (np.abs(r["variance"] - want_var)[wall] <= 1e-12 * want_var[wall]).all(), k
    assert abs(factor - 0.134) < 5e-4                            # the figure the real-frame test's expectation uses


def test_reference_reproduces_an_affine_light_under_a_moved_camera():
    """bilinear interpolation reproduces an affine function: after A -> B without noise every pixel with a history whose four
    taps were all accepted (W = 1; with a rejected tap the renormalised rest is no bilinear interpolation any more) holds the
    clean colour of the frame B -- a check of the reprojection that does not depend on the transcription's own geometry being
    repeated by the kernel"""
    for second in (cam_b, cam_c):
        (_, _, _, r1), (_, pl, clean, r2) = _sequence([cam_a(37, 23), second(37, 23)], 0.0, light=light_affine, dtype=np.float64)
        assert (r2["history"][r2["has"]] > 1).all()
        has = r2["has"] & (r2["weight"] > 1 - 1e-9)
        assert has.sum() > 0.7 * _valid(pl).sum()
        assert (np.abs(r2["linear"] - clean)[has] <= 1e-9 * np.abs(clean[has])).all()
        # a wrong reprojection would show: the same with the history shifted by one pixel does not reproduce the light
        hist = {}
        plA, _ = frame(cam_a(37, 23), 0, 0.0, light_affine, np.float64)
        ref_temporal(hist, cam_a(37, 23), plA)
        for key in ("d", "u", "N", "z", "n", "id"):
            hist[key] = np.roll(hist[key], 1, axis=1)
        r3 = ref_temporal(hist, second(37, 23), pl)
        assert np.abs(r3["linear"] - clean)[r3["has"] & (r3["weight"] > 1 - 1e-9)].max() > 1e-4


def test_reference_gives_disoccluded_wall_pixels_no_history():
    """A -> B: the wall behind the square as A saw it is new in B (the taps there hold the square: another id, another depth)"""
    for with_ids in (True, False):
        (camA, plA, _, _), (camB, plB, _, r) = _sequence([cam_a(37, 23), cam_b(37, 23)], 0.0, with_ids)
        # where B's wall pixels land in A's image: on the square?
        cs, old = cam_setup(camB), cam_setup(camA)
        P = cs["pos"] + plB["z"].astype(np.float64)[..., None] * pixel_rays(cs)
        q = (P - old["pos"]) @ old["M"]
        t = old["b"][2] / q[..., 2]
        fx, fy = (q[..., 0] * t - old["b"][0]) / old["u"] - 0.5, (q[..., 1] * t - old["b"][1]) / old["v"] - 0.5
        inside = (fx >= 0) & (fx <= 35) & (fy >= 0) & (fy <= 21)
        x0, y0 = np.clip(np.floor(fx), 0, 35).astype(int), np.clip(np.floor(fy), 0, 21).astype(int)
        all_square = np.ones(fx.shape, bool)
        for i in (0, 1):
            for j in (0, 1):
                all_square &= plA["object_id"][y0 + j, x0 + i] == 4
        hidden = (plB["object_id"] == 3) & inside & all_square
        assert hidden.sum() >= 5
        assert (r["history"][hidden] == 1).all() and not r["has"][hidden].any()
        assert (r["history"][(plB["object_id"] == 3) & r["has"]] == 2).all()


def test_reference_rejects_a_changed_id_and_a_turned_normal_and_reset_starts_anew():
    cam = cam_a(37, 23)
    pl, _ = frame(cam, 0, 0.0)
    hist = {}
    ref_temporal(hist, cam, pl)
    other = dict(pl, object_id=np.where(pl["object_id"] == 3, 7, pl["object_id"]).astype(np.int32))
    r = ref_temporal(dict(hist), cam, other)
    assert (r["history"][pl["object_id"] == 3] == 1).all() and (r["history"][pl["object_id"] == 4] == 2).all()
    r = ref_temporal(dict(hist), cam, other, with_ids=False)    # without the id plane the stored ids do not matter
    assert (r["history"][pl["object_id"] >= 0] == 2).all()
    turned = pl["normal"].copy()
    turned[pl["object_id"] == 4] = (0.6 * math.cos(0.4), 0.6 * math.sin(0.4), 0.8)     # |dn|^2 = 0.057 < 0.09: kept
    r = ref_temporal(dict(hist), cam, dict(pl, normal=turned))
    assert (r["history"][pl["object_id"] == 4] == 2).all()
    turned[pl["object_id"] == 4] = (0.0, 0.6, 0.8)              # |dn|^2 = 0.72: rejected
    r = ref_temporal(dict(hist), cam, dict(pl, normal=turned))
    assert (r["history"][pl["object_id"] == 4] == 1).all() and (r["history"][pl["object_id"] == 3] == 2).all()
    r = ref_temporal({}, cam, pl)                               # reset(): the history is empty
    assert (r["history"][pl["object_id"] >= 0] == 1).all() and not r["has"].any()


PAIRS = [("A,A,A", (cam_a, cam_a, cam_a)), ("A,B,C", (cam_a, cam_b, cam_c))]


def test_few_pixels_are_left_out_of_the_gpu_comparisons():
    """the condition on the cameras: at most 2 % of the valid pixels of any frame of any sequence the GPU tests use"""
    runs = [(name, cams, 37, 23) for name, cams in PAIRS] + [("A,B", (cam_a, cam_b), w, h) for w, h in SIZES[1:]]
    runs.append(("A,B affine", (cam_a, cam_b), 37, 23))
    for name, cams, w, h in runs:
        for with_ids in (True, False):
            seq = _sequence([c(w, h) for c in cams], 0.0 if "affine" in name else 0.3, with_ids)
            for k, (cam, pl, _, r) in enumerate(seq):
                valid = _valid(pl, with_ids)
                share = r["left_out"].sum() / max(1, valid.sum())
                assert share <= MAX_LEFT_OUT, (name, w, h, with_ids, k, share)


# ---- GPU: against the reference ---------------------------------------------------------------------------------
def _gate(got, want, s, delta, keep, what, floor):
    """|got - want| <= 2e-5 |want| + floor + delta_px * S on the kept pixels; returns the worst error / tolerance"""
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - want)[keep]
    tol = (2e-5 * np.abs(want) + floor + delta * s)[keep]
    worst = float((err / tol).max()) if err.size else 0.0
    print(f"temporal {what}: max |got-want| = {err.max() if err.size else 0:.3e}, worst err/tolerance = {worst:.4f}")
    assert (err <= tol).all(), (what, worst)
    return worst


def _run_against_reference(cams, w, h, with_ids, with_var, what, noise=0.3, light=light_smooth):
    """the same frames to a History on the GPU and to the reference, which carries its own history; compares after each step"""
    worst, old = 0.0, None
    with capi.History(0, w, h) as hst:
        for k, (cam, pl, clean, r) in enumerate(_sequence([c(w, h) for c in cams], noise, with_ids, with_var, light)):
            res = hst.accumulate(cam, pl["linear"], pl["normal"], pl["albedo"], pl["z"], return_history=True, **_planes_for(pl, with_ids, with_var))
            got, got_hist = res[0], res[-1]
            assert hst.frames == k + 1
            part = r["part"]
            keep = part & ~r["left_out"]
            assert r["left_out"].sum() <= MAX_LEFT_OUT * max(1, _valid(pl, with_ids).sum())
            delta = delta_px(old, cam, float(pl["z"][part].min())) if old is not None and part.any() else 0.0
            tag = f"{what} {w}x{h} ids={with_ids} var={with_var} step {k}"
            worst = max(worst, _gate(got, r["linear"], r["s_linear"], delta, keep, tag + " colour", 1e-6))
            worst = max(worst, _gate(got_hist, r["history"], r["s_history"], delta, keep, tag + " history", 1e-6))
            if with_var:
                worst = max(worst, _gate(res[1], r["variance"], r["s_variance"], delta, keep, tag + " variance", 1e-12))
                assert res[1][~part].tobytes() == pl["variance"][~part].tobytes()
            assert got[~part].tobytes() == pl["linear"][~part].tobytes() and (got_hist[~part] == 0).all()
            old = cam
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name,cams", PAIRS)
@pytest.mark.parametrize("with_ids,with_var", [(True, True), (False, True), (True, False), (False, False)])
def test_accumulation_against_the_reference_37x23(name, cams, with_ids, with_var):
    """The gate: the project's 2e-5 |want| + 1e-6 (variance: floor 1e-12, history: 1e-6) plus delta_px * S_p -- S_p the spread
    of the accepted taps' stored values, delta_px the bound derived in delta_px() above from the operation chain, not from what
    the GPU returns.  Measured on the MI355X: DESIGN 3."""
    _run_against_reference(cams, 37, 23, with_ids, with_var, name)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES[1:])
def test_accumulation_against_the_reference_at_small_sizes(w, h):
    for with_ids in (True, False):
        _run_against_reference((cam_a, cam_b), w, h, with_ids, True, "A,B")


@pytest.mark.gpu
def test_affine_light_is_reproduced_under_a_moved_camera():
    """the property of test_reference_reproduces_an_affine_light_under_a_moved_camera on the GPU, within the same gate and
    without the transcription: the yardstick is the clean colour of frame B itself (S_p and the pixels with a history are read
    from the reference, the expected values are not)"""
    w, h = 37, 23
    camA, camB = cam_a(w, h), cam_b(w, h)
    (_, plA, _, _), (_, plB, clean, r) = _sequence([camA, camB], 0.0, light=light_affine)
    with capi.History(0, w, h) as hst:
        hst.accumulate(camA, plA["linear"], plA["normal"], plA["albedo"], plA["z"], plA["object_id"])
        got, hist = hst.accumulate(camB, plB["linear"], plB["normal"], plB["albedo"], plB["z"], plB["object_id"], return_history=True)
    keep = r["has"] & (r["weight"] > 1 - 1e-6) & ~r["left_out"]     # all four taps accepted: see the CPU test
    assert keep.sum() > 0.7 * _valid(plB).sum() and (hist[keep] > 1).all()
    # the inputs are float32: clean itself is rounded (2^-24 relative, inside the 2e-5)
    _gate(got, clean.astype(np.float64), r["s_linear"], delta_px(camA, camB, float(plB["z"][r["part"]].min())), keep, "affine light A,B colour", 1e-6)


@pytest.mark.gpu
def test_invalid_nan_and_bad_variance_pixels_pass_through_and_leave_no_history():
    w, h = 37, 23
    cam = cam_a(w, h)
    pl, _ = frame(cam, 5, 0.3)
    lin, var = pl["linear"].copy(), pl["variance"].copy()
    inv = ~_valid(pl)
    lin[inv] = F([np.nan, -1e30, 7.5])[None]                    # invalid pixels hold anything, colour and variance
    var[inv] = F([-2.0, np.nan, 1e30])[None]
    lin[12, 8] = (np.nan, 0.3, 0.2)                             # valid pixels whose colour is not finite ...
    lin[5, 20, 1] = np.inf
    var[12, 8] = (0.5, np.nan, -1.0)                            # ... keep their variance too, whatever it holds
    bad = np.zeros((h, w), bool)
    bad[12, 8] = bad[5, 20] = True
    var[15:18, 6:9, 0], var[15:18, 6:9, 1], var[3, 30, 2] = np.nan, -3.0, np.inf       # bad components of pixels that take part: 0
    q = dict(pl, linear=lin, variance=var)
    nxt, _ = frame(cam, 6, 0.3)
    for with_ids in (True, False):
        valid = _valid(pl, with_ids)
        keep = valid & ~bad
        hist = {}
        r1 = ref_temporal(hist, cam, q, with_ids)
        r2 = ref_temporal(hist, cam, nxt, with_ids)
        with capi.History(0, w, h) as hst:
            got, got_var, n1 = hst.accumulate(cam, lin, pl["normal"], pl["albedo"], pl["z"], variance=var, return_history=True,
                                              object_id=pl["object_id"] if with_ids else None)
            got2, got_var2, n2 = hst.accumulate(cam, nxt["linear"], nxt["normal"], nxt["albedo"], nxt["z"], variance=nxt["variance"],
                                                return_history=True, object_id=nxt["object_id"] if with_ids else None)
        with capi.History(0, w, h) as hst:                      # the same with those components set to 0 beforehand
            zeroed = np.where(keep[..., None] & ~(np.isfinite(var) & (var > 0)), F(0), var)
            got0, got_var0 = hst.accumulate(cam, lin, pl["normal"], pl["albedo"], pl["z"], variance=zeroed,
                                            object_id=pl["object_id"] if with_ids else None)
        for m in (~valid, bad):                                 # bit for bit, NaN payloads included
            assert got[m].tobytes() == lin[m].tobytes() and got_var[m].tobytes() == var[m].tobytes() and (n1[m] == 0).all()
        assert (n1[keep] == 1).all() and np.isfinite(got[keep]).all() and np.isfinite(got_var[keep]).all()
        assert got0.tobytes() == got.tobytes() and got_var0[keep].tobytes() == got_var[keep].tobytes()
        _gate(got, r1["linear"], r1["s_linear"], 0.0, keep, f"pass-through ids={with_ids} step 0 colour", 1e-6)
        _gate(got_var, r1["variance"], r1["s_variance"], 0.0, keep, f"pass-through ids={with_ids} step 0 variance", 1e-12)
        # the next frame (same camera, every pixel finite): a pixel that passed through gave no history to the pixel that
        # reprojects onto it, and reaches no neighbour
        assert (n2[bad] == 1).all() and (n2[keep] == 2).all() and (n2[~valid] == 0).all()
        delta = delta_px(cam, cam, float(nxt["z"][valid].min()))
        k2 = valid & ~r2["left_out"]
        _gate(got2, r2["linear"], r2["s_linear"], delta, k2, f"pass-through ids={with_ids} step 1 colour", 1e-6)
        _gate(got_var2, r2["variance"], r2["s_variance"], delta, k2, f"pass-through ids={with_ids} step 1 variance", 1e-12)
        assert np.isfinite(got2[valid]).all() and np.isfinite(got_var2[valid]).all()


@pytest.mark.gpu
def test_camera_size_and_the_other_argument_checks_with_a_history():
    L = capi.lib()
    buf, cases, full = _arg_cases()
    with capi.History(0, 8, 8) as hst:
        cam = cam_a(8, 8)
        for what, p, pl in cases:
            assert L.rt_temporal(hst._h, C.byref(cam), C.byref(p), C.byref(pl)) == -1 and what in L.rt_last_error(), what
        p, pl = capi.temporal_params(), full()
        for bad in (cam_a(9, 8), cam_a(8, 7)):
            assert L.rt_temporal(hst._h, C.byref(bad), C.byref(p), C.byref(pl)) == -1 and b"the history 8 x 8" in L.rt_last_error()
            assert L.rt_temporal_device(hst._h, None, C.byref(bad), C.byref(p), C.byref(pl), 1) == -1
        assert hst.frames == 0                                  # nothing of this reached the GPU


@pytest.mark.gpu
def test_determinism_aliasing_entry_points_two_histories_and_reset():
    import torch
    w, h = 37, 23
    cams = [cam_a(w, h), cam_b(w, h), cam_c(w, h)]
    frames = [frame(c, 40 + k, 0.3)[0] for k, c in enumerate(cams)]
    big_cam = cam_b(90, 60)
    big, _ = frame(big_cam, 9, 0.3)

    def host_run(disturb=False):
        outs = []
        with capi.History(0, w, h) as hst, capi.History(0, 90, 60) as other:
            for cam, pl in zip(cams, frames):
                outs.append(hst.accumulate(cam, pl["linear"], pl["normal"], pl["albedo"], pl["z"], pl["object_id"], variance=pl["variance"],
                                           rgb8=True, return_history=True))
                if disturb:                                     # a history of another size on the same device, between the frames
                    other.accumulate(big_cam, big["linear"], big["normal"], big["albedo"], big["z"], big["object_id"])
        return outs

    first, again = host_run(), host_run(disturb=True)
    for a, b in zip(first, again):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
    assert first[0][0].tobytes() != first[2][0].tobytes() and (first[2][3] > 1).any()

    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    t = [{k: torch.from_numpy(np.array(v)).to(dev) for k, v in pl.items()} for pl in frames]
    mk = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
    torch.cuda.synchronize()
    with capi.History(0, w, h) as out_of_place, capi.History(0, w, h) as in_place:
        for k, (cam, tp) in enumerate(zip(cams, t)):
            ptrs = dict(normal_ptr=tp["normal"].data_ptr(), albedo_ptr=tp["albedo"].data_ptr(), z_ptr=tp["z"].data_ptr(),
                        object_id_ptr=tp["object_id"].data_ptr())
            out, out_var, hist, rgb8 = mk(h, w, 3), mk(h, w, 3), mk(h, w), mk(h, w, 3, dt=torch.uint8)
            out_of_place.accumulate_device(side.cuda_stream, cam, linear_ptr=tp["linear"].data_ptr(), out_ptr=out.data_ptr(),
                                           variance_ptr=tp["variance"].data_ptr(), out_variance_ptr=out_var.data_ptr(),
                                           history_ptr=hist.data_ptr(), rgb8_ptr=rgb8.data_ptr(), sync=False, **ptrs)
            lin2, var2 = tp["linear"].clone(), tp["variance"].clone()
            side.wait_stream(torch.cuda.current_stream(dev))
            in_place.accumulate_device(side.cuda_stream, cam, linear_ptr=lin2.data_ptr(), out_ptr=lin2.data_ptr(), variance_ptr=var2.data_ptr(),
                                       out_variance_ptr=var2.data_ptr(), sync=False, **ptrs)
            side.synchronize()
            want = first[k]
            assert out.cpu().numpy().tobytes() == want[0].tobytes() and out_var.cpu().numpy().tobytes() == want[1].tobytes()
            assert rgb8.cpu().numpy().tobytes() == want[2].tobytes() and hist.cpu().numpy().tobytes() == want[3].tobytes()
            assert lin2.cpu().numpy().tobytes() == want[0].tobytes() and var2.cpu().numpy().tobytes() == want[1].tobytes()
            assert tp["linear"].cpu().numpy().tobytes() == frames[k]["linear"].tobytes()
        assert out_of_place.frames == 3
        # reset(), then a frame: a fresh history's first frame
        out_of_place.reset()
        assert out_of_place.frames == 0
        tp, out, hist = t[0], mk(h, w, 3), mk(h, w)
        out_of_place.accumulate_device(side.cuda_stream, cams[0], linear_ptr=tp["linear"].data_ptr(), out_ptr=out.data_ptr(),
                                       variance_ptr=tp["variance"].data_ptr(), history_ptr=hist.data_ptr(), sync=True,
                                       normal_ptr=tp["normal"].data_ptr(), albedo_ptr=tp["albedo"].data_ptr(), z_ptr=tp["z"].data_ptr(),
                                       object_id_ptr=tp["object_id"].data_ptr())
        assert out.cpu().numpy().tobytes() == first[0][0].tobytes() and hist.cpu().numpy().tobytes() == first[0][3].tobytes()
        assert out_of_place.frames == 1


# ---- GPU: real frames -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_eight_accumulated_4spp_frames_come_closer_to_64spp():
    """cornell_gi.xml (live GI) at 96 x 72, reproducible mode: eight 4 spp frames, seeds 1..8, fixed camera, accumulated; the
    yardstick a 64 spp frame of another seed.  Expectation: the weight recursion (test_reference_error_variance_...) leaves
    0.134 of a frame's variance after 8 frames, and the target's own noise adds 4 / 64 of it to both sides:
    sqrt((0.134 + 0.0625) / (1 + 0.0625)) = 0.43.  Asserted: < 0.6 -- the margin is for the part of a 4 spp frame's error that
    repeats from seed to seed (the Halton positions inside the pixel are the same in every frame).  Measured on the MI355X:
    DESIGN 3; the denoised and the moving-camera ratios printed here are measured, not asserted."""
    s, cam = scenes.load_cornell_gi(96, 72)
    s.set_render_flags(capi.RENDER_REPRODUCIBLE)
    ref = s.render_outputs(cam, _gi_params(77, 64), planes=("linear", "object_id"))
    with capi.History(0, 96, 72) as hst, capi.History(0, 96, 72) as hst_d:
        for seed in range(1, 9):
            out = s.render_temporal(hst, cam, _gi_params(seed), denoise=False)
            assert "denoised" not in out and hst.frames == seed
        den = [s.render_temporal(hst_d, cam, _gi_params(seed)) for seed in range(1, 9)][-1]
    hit = out["object_id"] >= 0
    valid = hit & (ref["object_id"] >= 0)
    assert valid.mean() > 0.9 and (out["count"] == 0).all()
    assert (out["history"][hit] == 8).all() and (out["history"][~hit] == 0).all()
    rmse = lambda a: float(np.sqrt(((a[valid].astype(np.float64) - ref["linear"][valid]) ** 2).mean()))
    noisy, acc, dn = rmse(out["linear"]), rmse(out["accumulated"]), rmse(den["denoised"])
    assert den["accumulated"].tobytes() == out["accumulated"].tobytes() and den["denoised_rgb"].dtype == np.uint8
    assert out["accumulated"][~hit].tobytes() == out["linear"][~hit].tobytes()
    assert out["accumulated_variance"][hit].mean() < 0.25 * out["variance"][hit].mean()
    print(f"temporal cornell_gi 96x72: RMSE to 64 spp, frame 8 at 4 spp {noisy:.5f} -> 8 frames accumulated {acc:.5f} (ratio {acc / noisy:.3f}), "
          f"denoised on top {dn:.5f} (ratio {dn / noisy:.3f})")
    # the same with the camera translated by 1 % of the scene's width (0.3) between the frames
    with capi.History(0, 96, 72) as hst:
        for seed in range(1, 9):
            moving = s.render_temporal(hst, cam, _gi_params(seed))
            if seed < 8:
                cam.pos[0] += 0.3
    ref_m = s.render_outputs(cam, _gi_params(77, 64), planes=("linear", "object_id"))
    vm = (moving["object_id"] >= 0) & (ref_m["object_id"] >= 0)
    rm = lambda a: float(np.sqrt(((a[vm].astype(np.float64) - ref_m["linear"][vm]) ** 2).mean()))
    print(f"temporal cornell_gi 96x72, camera moving 0.3 a frame: 4 spp {rm(moving['linear']):.5f} -> accumulated {rm(moving['accumulated']):.5f} "
          f"(ratio {rm(moving['accumulated']) / rm(moving['linear']):.3f}), denoised on top {rm(moving['denoised']):.5f} "
          f"(ratio {rm(moving['denoised']) / rm(moving['linear']):.3f}), mean history {moving['history'][moving['object_id'] >= 0].mean():.2f}")
    assert acc / noisy < 0.6, (noisy, acc)


@pytest.mark.gpu
def test_cpp_shim_accumulation_equals_the_capi_one(tmp_path):
    exe = build_driver(tmp_path, "shim_temporal_driver")
    prefix = str(tmp_path / "f")
    r = subprocess.run([exe, scenes.CORNELL, prefix, "64", "48"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.split()[1] == str(64 * 48) and r.stdout.split()[-1] == "2", r.stdout
    s, cam = scenes.load_cornell(64, 48)
    s.set_render_flags(capi.RENDER_REPRODUCIBLE)
    with capi.History(0, 64, 48) as hst:
        p = capi.default_params(shade_model=capi.SHADE_P13, bounce=6, photon_count=0, min_sample=4, max_sample=8, threshold=1e-3, seed=11)
        one = s.render_temporal(hst, cam, p, denoise=False)
        cam.pos[0] = float(F(cam.pos[0]) + F(0.3))
        cam.pos[2] = float(F(cam.pos[2]) + F(0.1))
        p.seed = 12
        two = s.render_temporal(hst, cam, p, denoise=False)
    assert capi.image_read_pfm(prefix + "_acc1.pfm").tobytes() == one["accumulated"].tobytes()
    assert capi.image_read_pfm(prefix + "_acc2.pfm").tobytes() == two["accumulated"].tobytes()
    assert capi.image_read_pfm(prefix + "_accvar2.pfm").tobytes() == two["accumulated_variance"].tobytes()
    assert capi.image_read_pfm1(prefix + "_len2.pfm").tobytes() == two["history"].tobytes()
    assert (two["history"] > 1).mean() > 0.5 and np.abs(two["accumulated"] - two["linear"]).max() > 0
