"""Depth of field (include/rt_mi355x.h, "depth of field"): rt_dof_*, capi.DepthOfField, Scene.render_denoised / render_temporal
(depth_of_field=), the C++ shim's EnableDepthOfField() / DepthOfField().

ref_dof is a numpy transcription of the definition.  Its discrete decisions -- c, D, r, both maxima, the early out, the tap pixels
and whether a tap has a weight (cov > 0) -- are float32 in the stated order whatever `dtype` is; the weights and the colour sums are
taken in `dtype`.  float64 is the yardstick; with float32 numpy rounds every operation on its own, which is what a device does, and
the gate is held against that evaluation too, on the CPU.  out_coc, out_tiles and the pixels that pass through are compared bit for
bit.  The tap table is the library's (capi.dof_taps); A and the camera quantities are transcribed from the header's step 0.

Gate: C * 2^-24 * max(|c| over the centre and the pixel's live taps) + 1e-7, C counted in roundings (u = 2^-24 each).  The output is a
normalised average, out = S / W with S = sum w_k c_k, so an ABSOLUTE error dw_k of a weight moves it by dw_k (c_k - out) / W, at most
2 max|c| dw_k / W.  cov = clamp01((r_e - d) + 0.5) subtracts, so its error is absolute, and it enters w divided by r_e^2 (down to
0.25) and times R^2 / N: how much it matters depends on W, which may be as small as w_p = 1 / K^2.  Hence the count per pixel.
The inputs of a weight -- r_s, r_p, D_s, D_p, R, the tap pixel -- are float32 values both evaluations share: they carry no error.
  d        dx, dy and dx^2 + dy^2 are exact integers; one sqrt: relative u.
  behind   D_s - D_p: u; e: u; the quotient: u.  Inside the ramp (at most 1): 3u absolute; outside both sides clamp.
  r_e      min(rs, rp) - rs (at most K): u K; times behind: 3u K + u K; rs + that (at most K): u K.  dr_e <= 6u K.
  cov      r_e - d: dr_e + u d + u |r_e - d|, inside the ramp d <= K + 1 and |r_e - d| <= 1: 6u K + u (K + 2); + 0.5: u.
           dcov <= u (7 K + 3).
  r_e^2    relative 2 dr_e / r_e + u = u (12 K / r_e + 1).
  area     R * R: u; / N: u.  Relative 2u.
  w        area * cov: u; the division: u.  With g = area / r_e^2 (the weight at cov = 1):
           dw <= g (dcov + cov u (2 + 1 + 1 + 1 + 12 K / r_e)) <= g u (7 K + 8 + 12 K / r_e) =: u A_i.
  centre   q * q: u; 1 / that: u.  2u relative, 4u of max|c| at most.
  sums     n <= N + 1 terms: the products and additions of S n u, those of W (n - 1) u, the division u: below (2 N + 2) u max|c|.
  C = 2 N + 8 + 2 sum_i A_i / W, per pixel, from the float64 evaluation's r_e and W.

Against the renderer's own lens (test_stage_against_the_lens_render), measured on an MI355X, cornell.xml 96 x 72 at 256 spp, focused
on the teapot (focaldist 65, dof 3: A = 6.2 px, c from -3.5 on the floor's near edge to 1.2 on the back wall), RMSE in linear colour
against a lens render: a second lens render 0.0381 (e_noise), the pinhole render 0.0808 (e_pin), the stage on the pinhole render
0.0536 (e_post).  e_post / e_pin = 0.664 and e_noise / e_pin = 0.472 (what two lens renders differ by is the floor no stage can go
below).  The asserted bound is halfway between the measured ratio and 1."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from raytracing_folder_amd import capi
from tests import scenes
from tests.stage_support import F, U, assert_driver_usage, build_driver

DEFAULTS = dict(max_coc=16, samples=32, depth_extent=0.05, aperture_scale=1.0, focus=0.0)
JITTER = (0, 2, 3, 1)
FAR = F(1e30)


def camera(w, h, fov=40.0, focaldist=10.0, dof=0.0):
    cam = capi.Camera()
    cam.pos[:], cam.dir[:], cam.up[:] = (0, 0, 0), (0, 1, 0), (0, 0, 1)
    cam.fov, cam.focaldist, cam.dof, cam.width, cam.height = fov, focaldist, dof, w, h
    return cam


# ---- the transcription --------------------------------------------------------------------------------------------
def ref_setup(cam, aperture_scale=1.0, focus=0.0):
    """step 0: (A, fd, bx, by, u, v, l), float32 each"""
    W, H = cam.width, cam.height
    fov, l = F(cam.fov), F(cam.focaldist)
    fd = F(focus) if F(focus) != 0 else l
    t = math.tan(float(fov) / 2 * (math.pi / 180))
    A = F((float(F(aperture_scale)) * abs(float(F(cam.dof))) * H) / (2.0 * float(fd) * t))
    hh = F(float(F(2) * l) * math.tan(float(fov / F(2)) * (math.pi / 180)))
    ww = (hh * F(W)) / F(H)
    u, v = ww / F(W), -hh / F(H)
    bx, by = -ww / F(2) + u / F(2), hh / F(2) + v / F(2)
    return A, fd, F(bx), F(by), F(u), F(v), l


def ref_cos(cam):
    """cos(theta) of step 1 per pixel, float32 (H, W)"""
    _, _, bx, by, u, v, l = ref_setup(cam)
    Y, X = np.mgrid[0:cam.height, 0:cam.width]
    sx, sy = bx + (X.astype(F) + F(0.5)) * u, by + (Y.astype(F) + F(0.5)) * v
    return (l / np.sqrt((sx * sx + sy * sy) + l * l)).astype(F)


def ref_coc(z, cam, K, aperture_scale=1.0, focus=0.0):
    """step 1: (c, D, r), float32 (H, W) each"""
    A, fd = ref_setup(cam, aperture_scale, focus)[:2]
    z = np.asarray(z, F)
    with np.errstate(all="ignore"):
        valid = np.isfinite(z) & (z > 0) & (z < FAR)
        D = np.maximum(np.where(valid, z, F(1)) * ref_cos(cam), F(1e-6)).astype(F)
        c = (A * (F(1) - fd / D)).astype(F)
        c, D = np.where(valid, c, A).astype(F), np.where(valid, D, FAR).astype(F)
    return c, D, np.minimum(np.abs(c), F(K)).astype(F)


def ref_tiles(r, K):
    """steps 2 and 3: R per tile, float32 (TY, TX)"""
    H, W = r.shape
    TX, TY = -(-W // K), -(-H // K)
    pad = np.zeros((TY * K, TX * K), F)
    pad[:H, :W] = r
    tm = pad.reshape(TY, K, TX, K).max(axis=(1, 3))
    big = np.zeros((TY + 2, TX + 2), F)
    big[1:-1, 1:-1] = tm
    return np.max([big[1 + dy:1 + dy + TY, 1 + dx:1 + dx + TX] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0).astype(F)


def ref_dof(rgb, z, cam, dtype=np.float64, **kw):
    """the definition: a dict with out (in `dtype`), coc (float32 (H, W), the signed unclamped c), tiles (float32 (TY, TX), R),
    through (the pixels that pass unchanged), C (of the gate, per pixel), maxc (max|c| over the centre and the live taps) and
    counts of what the taps met"""
    p = dict(DEFAULTS, **kw)
    K, N = int(p["max_coc"]), int(p["samples"])
    dt = dtype
    rgb, z = np.asarray(rgb, F), np.asarray(z, F)
    H, W = z.shape
    assert (cam.width, cam.height) == (W, H)
    Y, X = np.mgrid[0:H, 0:W]
    Xf, Yf = X.astype(F), Y.astype(F)
    taps = capi.dof_taps(N)
    with np.errstate(all="ignore"):
        c, D, r = ref_coc(z, cam, K, p["aperture_scale"], p["focus"])
        tiles = ref_tiles(r, K)
        R = tiles[Y // K, X // K]
        early = R < F(0.5)
        fin_p = np.isfinite(rgb).all(axis=2)
        ext = F(p["depth_extent"])

        def weights(t, rs, Ds, d):
            """(cov, r_e) of a tap in the type `t`"""
            clamp01 = lambda a: np.minimum(np.maximum(a, t(0)), t(1))
            rp_, Dp_, rs, Ds = r.astype(t), D.astype(t), rs.astype(t), Ds.astype(t)
            e = t(ext) * np.maximum(np.minimum(Ds, Dp_), t(F(1e-6)))
            behind = clamp01((Ds - Dp_) / e)
            re = np.maximum(rs + behind * (np.minimum(rs, rp_) - rs), t(0.5))
            return clamp01((re - d) + t(0.5)), re, behind

        q = np.maximum(r, F(0.5)).astype(dt)
        wp = dt(1) / (q * q)
        base = np.where(fin_p[..., None], rgb, F(0))
        Wsum = wp.copy()
        S = wp[..., None] * base.astype(dt)
        area = (R.astype(dt) * R.astype(dt)) / dt(N)
        Acnt = np.zeros((H, W))
        maxc = np.abs(base).max(axis=2).astype(np.float64)
        anyhit = np.zeros((H, W), bool)
        j = np.asarray(JITTER)[(Y & 1) * 2 + (X & 1)]
        n = dict(outside=0, on_p=0, behind=0, front=0, ramp=0)
        gather = ~early & fin_p
        for i in range(N):
            ox, oy = taps[i]
            tx = np.choose(j, [ox, -oy, -ox, oy]).astype(F)
            ty = np.choose(j, [oy, ox, -oy, -ox]).astype(F)
            sxf = np.floor((Xf + R * tx) + F(0.5))
            syf = np.floor((Yf + R * ty) + F(0.5))
            inside = (sxf >= 0) & (sxf < W) & (syf >= 0) & (syf < H)
            sx, sy = np.where(inside, sxf, 0).astype(np.int64), np.where(inside, syf, 0).astype(np.int64)
            on_p = inside & (sx == X) & (sy == Y)
            cs = rgb[sy, sx]
            live = inside & ~on_p & np.isfinite(cs).all(axis=2)
            cs = np.where(live[..., None], cs, F(0))
            dx, dy = sxf - Xf, syf - Yf
            rs, Ds = r[sy, sx], D[sy, sx]
            cov32, _, b32 = weights(F, rs, Ds, np.sqrt(dx * dx + dy * dy).astype(F))
            hit = live & (cov32 > 0)
            cov, re, _ = weights(dt, rs, Ds, np.sqrt((dx * dx + dy * dy).astype(dt)))
            w = np.where(hit, (area * cov) / (re * re), dt(0)).astype(dt)
            Wsum = Wsum + w
            S = S + w[..., None] * cs.astype(dt)
            g = area.astype(np.float64) / (re.astype(np.float64) ** 2)
            Acnt += np.where(hit, g * (7.0 * K + 8.0 + 12.0 * K / re.astype(np.float64)), 0.0)
            maxc = np.maximum(maxc, np.abs(np.where(hit[..., None], cs, F(0))).max(axis=2))
            anyhit |= hit
            n["outside"] += int((gather & ~inside).sum()); n["on_p"] += int((gather & on_p).sum())
            n["behind"] += int((gather & live & (b32 == 1)).sum()); n["front"] += int((gather & live & (Ds < D)).sum())
            n["ramp"] += int((gather & live & (b32 > 0) & (b32 < 1)).sum())
        out = S / Wsum[..., None]
        through = early | ~fin_p | ~anyhit
        out = np.where(through[..., None], rgb.astype(dt), out)
        Cp = 2 * N + 8 + 2.0 * Acnt / Wsum.astype(np.float64)
        n["all_zero"] = int((gather & ~anyhit).sum())
        return dict(out=out, coc=c, tiles=tiles, through=through, early=early, C=Cp, maxc=maxc, r=r, n=n)


def over_gate(got, ref):
    """worst error / gate of a defocused plane against a float64 evaluation `ref`; the pixels that pass through must hold the same
    bytes"""
    want, through = ref["out"], ref["through"]
    got = np.asarray(got)
    assert got[through].astype(F).tobytes() == want[through].astype(F).tobytes()
    gate = (ref["C"] * U * ref["maxc"] + 1e-7)[..., None]
    with np.errstate(invalid="ignore"):                         # the pixels that pass through may hold a NaN or an inf
        err = np.abs(got.astype(np.float64) - want)[~through]
    assert np.isfinite(want[~through]).all() and np.isfinite(got[~through]).all()
    return float((err / np.broadcast_to(gate, want.shape)[~through]).max()) if err.size else 0.0


# ---- the frames -------------------------------------------------------------------------------------------------------
CASES = [(37, 23, 8, 32), (16, 16, 16, 32), (70, 41, 32, 64), (3, 2, 2, 8), (130, 18, 5, 32)]      # (W, H, K, N)
CASE_IDS = [f"{w}x{h}-K{k}" for w, h, k, _ in CASES]
FOCUS = 10.0


def frame(w, h, K, seed=1):
    """(rgb, z, cam) of a synthetic frame, fov 40, focused at 10 with A = 1.5 K: from the left an in-focus band (D = the focus
    distance, 2.5 tiles wide or half the frame), a near band (|c| = 2.25 K, clamped) and a far band whose depth rises by 1% a
    pixel (inside the depth_extent ramp) and with the row (c from 0.25 K to over K); in the right half a row of 1e30 and a few
    pixels each of NaN, inf, 0 and negative z and NaN / inf colours"""
    rng = np.random.default_rng(seed)
    rgb = rng.uniform(0.0, 4.0, (h, w, 3)).astype(F)
    A_want = 1.5 * K
    dof = A_want * 2.0 * FOCUS * math.tan(math.radians(20.0)) / h
    cam = camera(w, h, 40.0, FOCUS, dof)
    cs = ref_cos(cam)
    Y, X = np.mgrid[0:h, 0:w]
    x_focus = min(int(2.5 * K), w // 2)
    x_near = x_focus + max(1, (w - x_focus) // 3)
    z = (F(FOCUS) / cs).astype(F)
    z = np.where((X >= x_focus) & (X < x_near), F(4.0) / cs, z)
    far = F(12.0) * (F(1) + F(0.01) * (X - x_near).astype(F)) * (F(1) + F(3.0) * Y.astype(F) / F(max(h - 1, 1)))
    z = np.where(X >= x_near, far, z).astype(F)
    if w * h >= 64:
        z[h // 2, w // 2:] = FAR
        at = [(h // 4, w // 2 + k) for k in range(min(6, w - w // 2))]
        for (yy, xx), v in zip(at, (np.nan, np.inf, 0.0, -3.0)):
            z[yy, xx] = v
        if len(at) >= 6:
            rgb[at[4]] = (np.nan, 1.0, 1.0)
            rgb[at[5]] = (1.0, np.inf, 1.0)
    return rgb, z, cam


_REF = {}


def reference(case, dtype=np.float64):
    """the transcription of frame(...) of one of CASES, computed once and shared"""
    key = (case, dtype)
    if key not in _REF:
        w, h, K, N = case
        _REF[key] = ref_dof(*frame(w, h, K), dtype=dtype, max_coc=K, samples=N)
    return _REF[key]


# ---- without a GPU -------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("rt_dof_create", "rt_dof_destroy", "rt_dof_default_params", "rt_dof_tiles", "rt_dof_taps", "rt_dof_device", "rt_dof_host")


def test_new_symbols_struct_layout_and_defaults():
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert L.rt_abi_version() == 4
    assert [f[0] for f in capi.DofParams._fields_] == ["struct_size", "max_coc", "samples", "depth_extent", "aperture_scale", "focus"]
    assert [f[0] for f in capi.DofPlanes._fields_] == ["struct_size", "rgb_linear", "z", "out", "out_coc", "out_tiles"]
    assert C.sizeof(capi.DofParams) == 24 and C.sizeof(capi.DofPlanes) == 48
    p = capi.DofParams()
    L.rt_dof_default_params(C.byref(p))
    assert p.struct_size == 24
    for k, v in DEFAULTS.items():
        assert getattr(p, k) == (v if k in ("max_coc", "samples") else F(v)), k
    L.rt_dof_default_params(None)                               # ignored
    L.rt_dof_destroy(None)                                      # ignored
    with pytest.raises(TypeError):
        capi.dof_params(shutter=0.5)
    assert capi.dof_params(samples=8, focus=3.0).samples == 8
    # the existing structs did not grow
    assert C.sizeof(capi.MotionBlurParams) == 20 and C.sizeof(capi.MotionBlurPlanes) == 48 and C.sizeof(capi.Camera) == 56
    assert C.sizeof(capi.BloomParams) == 28 and C.sizeof(capi.ToneMapParams) == 52 and C.sizeof(capi.Outputs) == 72


def test_tiles_equal_ceil_and_the_tap_table():
    for w, h in [(1, 1), (37, 23), (64, 64), (130, 18), (1920, 1080), (1, 4096), (7, 1)]:
        for K in (2, 3, 5, 8, 16, 31, 32):
            assert capi.dof_tiles(w, h, K) == (math.ceil(w / K), math.ceil(h / K)), (w, h, K)
    assert capi.dof_tiles(1920, 1080) == (120, 68)
    L = capi.lib()
    assert L.rt_dof_tiles(0, 4, 16, None, None) == -1 and b"bad image size" in L.rt_last_error()
    for bad in (1, 33, 0, -2):
        assert L.rt_dof_tiles(4, 4, bad, None, None) == -1 and b"max_coc" in L.rt_last_error()
    assert L.rt_dof_tiles(4, 4, 2, None, None) == 0
    for N in (8, 9, 32, 33, 64):
        t = capi.dof_taps(N)
        assert t.dtype == np.float32 and t.shape == (N, 2) and t.tobytes() == capi.dof_taps(N).tobytes()
        rad = np.hypot(t[:, 0].astype(np.float64), t[:, 1].astype(np.float64))
        want = np.sqrt((np.arange(N) + 0.5) / N)
        assert (rad < 1.0).all() and (np.abs(rad - want) <= np.spacing(want.astype(F)).astype(np.float64)).all(), N
        phi = np.arange(N) * (math.pi * (3.0 - math.sqrt(5.0)))
        assert np.abs(t - np.stack([want * np.cos(phi), want * np.sin(phi)], axis=1)).max() <= 2.0 ** -23
    buf = np.zeros(130, np.float32)
    for bad in (7, 65, 0, -1):
        assert L.rt_dof_taps(bad, buf.ctypes.data) == -1 and b"samples" in L.rt_last_error()
    assert L.rt_dof_taps(8, None) == -1


def _arg_cases():
    """(what the message holds, the status, camera, params, planes) of every refusal that needs no object"""
    n = 8 * 8
    buf = np.zeros(n * 8 + 64, np.float32)
    ptr = buf.ctypes.data
    full = lambda **kw: capi.DofPlanes(**{**dict(rgb_linear=ptr, z=ptr + n * 12, out=ptr + n * 16, out_coc=ptr + n * 28, out_tiles=ptr + n * 32), **kw})
    good = lambda **kw: camera(8, 8, **{**dict(dof=0.5), **kw})
    nan, inf = float("nan"), float("inf")
    cases_ = []
    for bad in (0, 23, 28):
        p = capi.dof_params()
        p.struct_size = bad
        cases_.append((b"struct_size", -1, good(), p, full()))
    pl = full()
    pl.struct_size += 8
    cases_.append((b"struct_size", -1, good(), capi.dof_params(), pl))
    for bad in (1, 0, 33, -4):
        cases_.append((b"max_coc is", -1, good(), capi.dof_params(max_coc=bad), full()))
    for bad in (7, 0, 65, -3):
        cases_.append((b"samples is", -1, good(), capi.dof_params(samples=bad), full()))
    for bad in (0.0, 5e-4, -1.0, nan, inf):
        cases_.append((b"depth_extent", -1, good(), capi.dof_params(depth_extent=bad), full()))
    for bad in (-0.5, nan, inf):
        cases_.append((b"aperture_scale", -1, good(), capi.dof_params(aperture_scale=bad), full()))
    for bad in (-1.0, nan, inf, 1e21):
        cases_.append((b"focus must", -1, good(), capi.dof_params(focus=bad), full()))
    for name in ("rgb_linear", "z", "out"):
        cases_.append((b"are required", -1, good(), capi.dof_params(), full(**{name: None})))
    for bad in (0.0, 180.0, -30.0, nan):
        cases_.append((b"fov", -1, good(fov=bad), capi.dof_params(), full()))
    for bad in (nan, inf):
        cases_.append((b"dof must be finite", -1, good(dof=bad), capi.dof_params(), full()))
    for bad in (0.0, -2.0, nan, inf):
        cases_.append((b"focaldist", -1, good(focaldist=bad), capi.dof_params(), full()))
    cases_.append((b"not finite", -1, good(dof=3e38, focaldist=1e-20, fov=1e-3), capi.dof_params(), full()))
    for w_, h_ in ((0, 8), (8, 0), (-3, 8)):
        cam = good()
        cam.width, cam.height = w_, h_
        cases_.append((b"bad image size", -1, cam, capi.dof_params(), full()))
    cam = good()
    cam.width, cam.height = 1 << 16, (1 << 14) + 1
    cases_.append((b"2^30", -6, cam, capi.dof_params(), full()))
    for over in (dict(out=ptr), dict(out=ptr + 12), dict(out=ptr + n * 12 - 4), dict(z=ptr), dict(out_coc=ptr + n * 16), dict(out_tiles=ptr + n * 28 + n * 4 - 4)):
        cases_.append((b"overlap", -1, good(), capi.dof_params(max_coc=2), full(**over)))
    return buf, cases_, full, good


def test_argument_checks_come_before_any_gpu_call():
    """every check but the camera's size against the object's is reached with a NULL object, so it is reached without a device"""
    L = capi.lib()
    buf, cases_, full, good = _arg_cases()
    for what, status, cam, p, pl in cases_:
        for st in (L.rt_dof_host(None, C.byref(cam), C.byref(p), C.byref(pl)), L.rt_dof_device(None, None, C.byref(cam), C.byref(p), C.byref(pl), 1)):
            assert st == status and what in L.rt_last_error(), (what, st, L.rt_last_error())
    cam, p, pl = good(), capi.dof_params(), full()
    for args in ((None, C.byref(p), C.byref(pl)), (C.byref(cam), None, C.byref(pl)), (C.byref(cam), C.byref(p), None)):
        assert L.rt_dof_host(None, *args) == -1 and L.rt_dof_device(None, None, *args, 1) == -1
    assert L.rt_dof_host(None, C.byref(cam), C.byref(p), C.byref(pl)) == -1 and b"rt_dof is NULL" in L.rt_last_error()
    for ok in (dict(max_coc=2), dict(max_coc=32), dict(samples=8), dict(samples=64), dict(depth_extent=1e-3), dict(aperture_scale=0.0), dict(focus=1e20),
               dict(focus=1e-3)):
        q = capi.dof_params(**ok)                               # the ends of the ranges pass every check up to the object
        assert L.rt_dof_host(None, C.byref(cam), C.byref(q), C.byref(pl)) == -1 and b"rt_dof is NULL" in L.rt_last_error(), ok
    neg = good(dof=-0.5, focaldist=0.0)                         # |dof| is taken; focaldist is not looked at when focus is given
    assert L.rt_dof_host(None, C.byref(neg), C.byref(capi.dof_params(focus=2.0)), C.byref(pl)) == -1 and b"rt_dof is NULL" in L.rt_last_error()
    h = C.c_void_p()
    for w_, h_ in ((0, 8), (8, 0), (-3, 8)):
        assert L.rt_dof_create(0, w_, h_, C.byref(h)) == -1 and b"bad image size" in L.rt_last_error() and not h
    assert L.rt_dof_create(0, 8, 8, None) == -1
    assert L.rt_dof_create(0, 1 << 16, (1 << 14) + 1, C.byref(h)) == -6 and b"2^30" in L.rt_last_error() and not h
    if capi.device_count() == 0:                                # ... and RT_ERR_NO_DEVICE comes after all of them
        assert L.rt_dof_create(0, 8, 8, C.byref(h)) == -3 and not h
        with pytest.raises(capi.RtError) as err:
            capi.DepthOfField(0, 8, 8)
        assert err.value.status == -3


def test_shim_driver_builds_against_the_header(tmp_path):
    assert_driver_usage(build_driver(tmp_path, "shim_dof_driver"))


def test_frames_hold_what_the_tests_rely_on():
    total = dict(outside=0, on_p=0, behind=0, front=0, ramp=0, all_zero=0)
    for case in CASES:
        w, h, K, N = case
        ref = reference(case)
        rgb, z, cam = frame(w, h, K)
        assert np.abs(ref["coc"]).max() > K and np.abs(ref["coc"]).min() < 0.5, case       # |c| spans 0 to beyond K
        assert ref["tiles"].shape == capi.dof_tiles(w, h, K)[::-1]
        for k in total:
            total[k] += ref["n"][k]
        if w * h >= 64:
            assert (z == FAR).sum() >= 1 and np.isnan(z).sum() == 1 and np.isinf(z).sum() == 1 and (z == 0).sum() == 1 and (z < 0).sum() == 1
            assert (~np.isfinite(rgb)).any(axis=2).sum() == (2 if w - w // 2 >= 6 else 0)
            bad = ~np.isfinite(z) | (z <= 0) | (z >= FAR)
            assert (ref["coc"][bad] == ref_setup(cam)[0]).all()
        if (w, h) in ((37, 23), (130, 18)):                     # pixels below and above the early out
            assert ref["early"].any() and not ref["early"].all(), case
            assert (~ref["through"]).any()
    assert reference(CASES[3])["n"]["outside"] > 0 and not reference(CASES[3])["early"].any()        # 3 x 2: the taps clip
    assert all(v > 0 for v in total.values()), total


def test_reference_returns_the_input_where_nothing_is_out_of_focus():
    for case in CASES:
        w, h, K, N = case
        rgb, z, cam = frame(w, h, K)
        sharp = (F(FOCUS) / ref_cos(cam)).astype(F)
        for dt in (np.float32, np.float64):
            for z_, cam_, kw in ((z, camera(w, h, 40.0, FOCUS, 0.0), {}), (z, cam, dict(aperture_scale=0.0)), (sharp, cam, {})):
                ref = ref_dof(rgb, z_, cam_, dt, max_coc=K, samples=N, **kw)
                assert ref["early"].all() and ref["out"].astype(F).tobytes() == rgb.tobytes(), (case, kw)
        pulled = ref_dof(rgb, sharp, cam, max_coc=K, samples=N, focus=4.0)      # the same frame with the focus pulled is not
        assert not pulled["early"].any()


def test_reference_keeps_a_constant_colour_under_random_depth():
    for w, h, K, N in ((37, 23, 8, 32), (70, 41, 32, 64)):
        _, _, cam = frame(w, h, K)
        z = (10.0 ** np.random.default_rng(3).uniform(0.3, 1.7, (h, w))).astype(F)
        rgb = np.broadcast_to(np.array([3.0, 0.5, 0.125], F), (h, w, 3)).copy()
        ref = ref_dof(rgb, z, cam, max_coc=K, samples=N)
        assert not ref["through"].all()
        assert (np.abs(ref["out"] - rgb) <= 256 * 2.0 ** -53 * rgb).all()
        out32 = ref_dof(rgb, z, cam, np.float32, max_coc=K, samples=N)["out"]
        assert (np.abs(out32 - rgb) <= (2 * N + 8) * U * rgb).all()          # equal colours: the weights' errors cancel


def test_reference_nan_pixel_stays_and_changes_no_other():
    w, h, K, N = CASES[0]
    rgb, z, cam = frame(w, h, K)
    bad = ~np.isfinite(rgb).all(axis=2)
    assert bad.sum() == 2
    other = rgb.copy()
    other[bad] = (np.inf, -np.inf, np.nan)
    a, b = ref_dof(rgb, z, cam, max_coc=K, samples=N)["out"], ref_dof(other, z, cam, max_coc=K, samples=N)["out"]
    assert a[bad].astype(F).tobytes() == rgb[bad].tobytes() and np.isfinite(a[~bad]).all()
    assert a[~bad].tobytes() == b[~bad].tobytes()               # what the bad pixel holds reaches no other pixel


def _square_frame(w=48, h=40, K=8):
    rgb = np.random.default_rng(2).uniform(0.0, 4.0, (h, w, 3)).astype(F)
    cam = camera(w, h, 40.0, FOCUS, 1.5 * K * 2.0 * FOCUS * math.tan(math.radians(20.0)) / h)
    sq = np.zeros((h, w), bool)
    sq[12:28, 14:34] = True
    z = np.where(sq, F(FOCUS) / ref_cos(cam), F(40.0)).astype(F)
    return rgb, z, cam, sq


def test_reference_in_focus_square_stays_sharp_in_front_of_a_blurred_background():
    rgb, z, cam, sq = _square_frame()
    ref = ref_dof(rgb, z, cam, max_coc=8)
    assert not ref["early"].any() and ref["r"][sq].max() < 0.5 and ref["r"][~sq].min() > 4.0
    assert ref["out"][sq].astype(F).tobytes() == rgb[sq].tobytes() and ref["through"][sq].all()
    assert not ref["through"][~sq].any() and (np.abs(ref["out"][~sq] - rgb[~sq]).max(axis=1) > 1e-3).all()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_counted_gate_holds_for_a_float32_evaluation(case):
    w, h, K, N = case
    want, got = reference(case), reference(case, np.float32)
    assert got["coc"].tobytes() == want["coc"].tobytes() and got["tiles"].tobytes() == want["tiles"].tobytes()
    assert (got["through"] == want["through"]).all()
    worst = over_gate(got["out"], want)                         # every pixel: none is left out
    print(f"dof float32 evaluation {w}x{h} K {K} N {N}: worst error / gate {worst:.3f}, largest C {want['C'][~want['through']].max(initial=0):.0f}")
    assert worst <= 1.0


# ---- on the GPU ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_device_against_the_float64_transcription(case):
    w, h, K, N = case
    rgb, z, cam = frame(w, h, K)
    keep = [a.copy() for a in (rgb, z)]
    ref = reference(case)
    with capi.DepthOfField(0, w, h) as d:
        out, coc, tiles = d.apply(rgb, z, cam, return_coc=True, return_tiles=True, max_coc=K, samples=N)
        again = d.apply(rgb, z, cam, return_coc=True, return_tiles=True, max_coc=K, samples=N)
    assert coc.tobytes() == ref["coc"].tobytes() and tiles.tobytes() == ref["tiles"].tobytes()
    worst = over_gate(out, ref)
    print(f"dof {w}x{h} K {K} N {N}: worst error / gate {worst:.3f}")
    assert worst <= 1.0
    for a, b in zip((out, coc, tiles), again):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(keep, (rgb, z)):
        assert a.tobytes() == b.tobytes()


# (w, h, K) at the edges of the tile-gather geometry (csrc/rt_tile_gather.h; G = the tiles along a gather workgroup's square):
# the smallest image; narrower than one tile, one tile column, G = 1; G = 8 with a ragged last square and tile in x and one tile
# row; G = 3, a square of 15 pixels, ragged in both axes; the first K with G = 1, one workgroup of 81 pixels; everything divides;
# one pixel over in both axes
GEOMETRY = [(1, 1, 2), (3, 70, 32), (70, 3, 2), (33, 17, 5), (31, 33, 9), (64, 48, 8), (65, 49, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", GEOMETRY, ids=lambda s: f"{s[0]}x{s[1]}-K{s[2]}")
def test_device_at_the_edges_of_the_tile_geometry(shape):
    w, h, K = shape
    rgb, z, cam = frame(w, h, K)
    ref = reference((w, h, K, 32))
    with capi.DepthOfField(0, w, h) as d:
        out, coc, tiles = d.apply(rgb, z, cam, return_coc=True, return_tiles=True, max_coc=K, samples=32)
    assert coc.shape == ref["coc"].shape and coc.tobytes() == ref["coc"].tobytes()
    assert tiles.shape == ref["tiles"].shape and tiles.tobytes() == ref["tiles"].tobytes()
    worst = over_gate(out, ref)
    print(f"dof {w}x{h} K {K}: worst error / gate {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.gpu
def test_exact_properties_on_the_device():
    import torch
    case = CASES[0]
    w, h, K, N = case
    rgb, z, cam = frame(w, h, K)
    tx, ty = capi.dof_tiles(w, h, K)
    L = capi.lib()
    with capi.DepthOfField(0, w, h) as d:
        first = d.apply(rgb, z, cam, return_coc=True, return_tiles=True, max_coc=K, samples=N)
        # the early-out cases return the input bytes
        sharp = (F(FOCUS) / ref_cos(cam)).astype(F)
        assert d.apply(rgb, z, camera(w, h, 40.0, FOCUS, 0.0), max_coc=K).tobytes() == rgb.tobytes()
        assert d.apply(rgb, z, cam, max_coc=K, aperture_scale=0.0).tobytes() == rgb.tobytes()
        assert d.apply(rgb, sharp, cam, max_coc=K).tobytes() == rgb.tobytes()
        assert d.apply(rgb, sharp, cam, max_coc=K, focus=4.0).tobytes() != rgb.tobytes()
        # apply_device on torch tensors, in stream order without a sync
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(device=dev)
        src, dep = torch.from_numpy(rgb).to(dev), torch.from_numpy(z).to(dev)
        out, out2 = torch.zeros_like(src), torch.zeros_like(src)
        coc = torch.zeros((h, w), dtype=torch.float32, device=dev)
        tiles = torch.zeros((ty, tx), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        ptrs = dict(linear_ptr=src.data_ptr(), z_ptr=dep.data_ptr())
        d.apply_device(side.cuda_stream, cam, out_ptr=out.data_ptr(), coc_ptr=coc.data_ptr(), tiles_ptr=tiles.data_ptr(), max_coc=K, samples=N, **ptrs)
        with torch.cuda.stream(side):
            doubled = out * 2                                   # behind the stage on the same stream, no sync between
        d.apply_device(side.cuda_stream, cam, out_ptr=out2.data_ptr(), sync=True, max_coc=K, samples=N, **ptrs)
        side.synchronize()
        assert out.cpu().numpy().tobytes() == first[0].tobytes() == out2.cpu().numpy().tobytes()
        assert doubled.cpu().numpy().tobytes() == (first[0] * F(2)).tobytes()
        assert coc.cpu().numpy().tobytes() == first[1].tobytes() and tiles.cpu().numpy().tobytes() == first[2].tobytes()
        for t, a in ((src, rgb), (dep, z)):                     # the source planes are as they were
            assert t.cpu().numpy().tobytes() == a.tobytes()
        with pytest.raises(capi.RtError) as err:
            d.apply_device(side.cuda_stream, cam, out_ptr=src.data_ptr(), **ptrs)
        assert err.value.status == -1 and b"overlap" in L.rt_last_error()
        # another max_coc and samples on the same object: nothing is reallocated, and the first call's result comes back after
        for K2, N2 in ((2, 8), (32, 64), (5, 17)):
            got = d.apply(rgb, z, cam, return_tiles=True, max_coc=K2, samples=N2)
            ref = ref_dof(rgb, z, cam, max_coc=K2, samples=N2)
            assert got[1].tobytes() == ref["tiles"].tobytes() and over_gate(got[0], ref) <= 1.0, (K2, N2)
        assert d.apply(rgb, z, cam, max_coc=K, samples=N).tobytes() == first[0].tobytes()
        # a constant colour is kept, whatever the depth
        flat = np.broadcast_to(np.array([3.0, 0.5, 0.125], F), (h, w, 3)).copy()
        got = d.apply(flat, z, cam, max_coc=K, samples=64)
        assert (np.abs(got - flat) <= (2 * 64 + 8) * U * flat).all()
    # the in-focus square in front of a blurred background
    rgb, z, cam, sq = _square_frame()
    with capi.DepthOfField(0, cam.width, cam.height) as d:
        out = d.apply(rgb, z, cam, max_coc=8)
    assert out[sq].tobytes() == rgb[sq].tobytes() and (np.abs(out[~sq] - rgb[~sq]).max(axis=1) > 1e-3).all()


@pytest.mark.gpu
def test_argument_checks_with_an_object():
    import torch
    L = capi.lib()
    n = 8 * 8
    t = torch.zeros((n * 10,), dtype=torch.float32, device="cuda:0")
    ptr = t.data_ptr()
    p = capi.dof_params(max_coc=2)
    good = dict(rgb_linear=ptr, z=ptr + n * 12, out=ptr + n * 16, out_coc=ptr + n * 28, out_tiles=ptr + n * 32)
    cam = camera(8, 8, dof=0.5)
    with capi.DepthOfField(0, 8, 8) as d:
        _, cases_, _, _ = _arg_cases()
        for what, status, bad_cam, bad_p, pl in cases_:         # the same refusals with an object
            assert L.rt_dof_host(d._h, C.byref(bad_cam), C.byref(bad_p), C.byref(pl)) == status and what in L.rt_last_error(), what
        m = 16 * 9                                              # planes apart for the largest of these cameras
        wide = torch.zeros((m * 10,), dtype=torch.float32, device="cuda:0")
        wp = wide.data_ptr()
        apart = capi.DofPlanes(rgb_linear=wp, z=wp + m * 12, out=wp + m * 16, out_coc=wp + m * 28, out_tiles=wp + m * 32)
        for size in ((8, 9), (16, 8), (4, 4)):                  # the camera's size differs from the object's
            other = camera(*size, dof=0.5)
            assert L.rt_dof_device(d._h, None, C.byref(other), C.byref(p), C.byref(apart), 1) == -1
            assert b"the rt_dof 8 x 8" in L.rt_last_error(), size
        assert L.rt_dof_device(d._h, None, C.byref(cam), C.byref(p), C.byref(capi.DofPlanes(**good)), 1) == 0
        assert L.rt_dof_device(d._h, None, C.byref(cam), C.byref(p), C.byref(capi.DofPlanes(**dict(good, out_coc=None, out_tiles=None))), 1) == 0
    # (an rt_dof is on one device and its entry points name no other: the planes are that device's, as for rt_motion_blur)


def _params(seed, spp=None):
    kw = dict(min_sample=spp, max_sample=spp) if spp else dict(min_sample=4, max_sample=8)
    return capi.default_params(shade_model=capi.SHADE_P13, bounce=6, photon_count=0, threshold=1e-3, seed=seed, **kw)


LENS_FOCUS, LENS_DOF = 65.0, 3.0        # cornell.xml from (0, -60, 12): the teapot in focus, the spheres nearer, the back wall beyond


def _lens_camera(w, h):
    s, cam = scenes.load_cornell(w, h)
    cam.focaldist, cam.dof = LENS_FOCUS, LENS_DOF
    return s, cam


def _same_arrays(a, b, but=()):
    assert set(a) == set(b) | set(but)
    for k, v in b.items():
        if isinstance(v, np.ndarray):
            assert a[k].tobytes() == v.tobytes(), k


@pytest.mark.gpu
def test_render_chain_with_a_depth_of_field():
    """cornell.xml at 96 x 72, reproducible mode: render_denoised and render_temporal with depth_of_field="""
    w, h = 96, 72
    s, cam = _lens_camera(w, h)
    s.set_render_flags(capi.RENDER_REPRODUCIBLE)
    pin = capi._copy_camera(cam)
    pin.dof = 0.0
    with capi.DepthOfField(0, w, h) as d, capi.MotionBlur(0, w, h) as mb, capi.Bloom(0, w, h) as bl, capi.Exposure(0) as exp, \
            capi.History(0, w, h) as hst, capi.History(0, w, h) as hst_pin, capi.History(0, w, h) as hst_a, capi.History(0, w, h) as hst_b:
        one = s.render_denoised(cam, _params(11), depth_of_field=d)
        sharp = s.render_denoised(pin, _params(11))
        _same_arrays(one, sharp, but=("defocused", "coc"))      # the planes are the pinhole render's: z, object_id, ... and denoised
        assert cam.dof == F(LENS_DOF)                           # the caller's camera is as it was
        blurred, coc = d.apply(one["denoised"], one["z"], cam, return_coc=True)
        assert one["defocused"].tobytes() == blurred.tobytes() and one["coc"].tobytes() == coc.tobytes()
        assert (one["defocused"] != one["denoised"]).any() and np.abs(coc).max() > 1.0
        kw = dict(max_coc=8, samples=16, aperture_scale=2.0)
        two = s.render_denoised(cam, _params(11), depth_of_field=d, dof_kw=kw, bloom=bl)
        assert two["defocused"].tobytes() == d.apply(two["denoised"], two["z"], cam, **kw).tobytes()
        assert two["bloomed"].tobytes() == bl.apply(two["defocused"]).tobytes()
        # without the stage the lens path is what it was, and None is no stage
        lens, lens_none = s.render_denoised(cam, _params(11)), s.render_denoised(cam, _params(11), depth_of_field=None, dof_kw=None)
        _same_arrays(lens, lens_none)
        assert lens["z"].tobytes() != sharp["z"].tobytes()
        # the temporal chain: accumulate -> denoise -> depth of field -> motion blur -> bloom -> tone map
        mkw = dict(shutter=1.0, max_blur=8)
        for seed in (11, 12):
            t = s.render_temporal(hst, cam, _params(seed), moving=True, depth_of_field=d, motion_blur=mb, motion_blur_kw=mkw, bloom=bl, exposure=exp)
            tp = s.render_temporal(hst_pin, pin, _params(seed), moving=True)
            _same_arrays(t, tp, but=("defocused", "coc", "motion_blurred", "bloomed", "display_rgb"))
            assert t["defocused"].tobytes() == d.apply(t["denoised"], t["z"], cam).tobytes()
            assert t["motion_blurred"].tobytes() == mb.apply(t["defocused"], t["motion"], t["z"], **mkw).tobytes()
            assert (t["defocused"] != t["denoised"]).any()
            if seed == 11:                                      # exp held no metered frame when the first frame was bloomed
                assert t["bloomed"].tobytes() == bl.apply(t["motion_blurred"]).tobytes()
            assert t["display_rgb"].shape == (h, w, 3)
            a, b = s.render_temporal(hst_a, cam, _params(seed), moving=True), s.render_temporal(hst_b, cam, _params(seed), moving=True, depth_of_field=None)
            _same_arrays(a, b)
        three = s.render_temporal(hst, cam, _params(13), denoise=False, depth_of_field=d)
        assert "denoised" not in three and three["defocused"].tobytes() == d.apply(three["accumulated"], three["z"], cam).tobytes()


@pytest.mark.gpu
def test_cpp_shim_defocused_equals_the_capi_one(tmp_path):
    exe = build_driver(tmp_path, "shim_dof_driver")
    prefix = str(tmp_path / "f")
    w, h, K = 64, 48, 8
    r = subprocess.run([exe, scenes.CORNELL, prefix, str(w), str(h), str(LENS_FOCUS), str(LENS_DOF), str(K)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    s, cam = _lens_camera(w, h)
    s.set_render_flags(capi.RENDER_REPRODUCIBLE)
    with capi.DepthOfField(0, w, h) as d:
        one = s.render_denoised(cam, _params(11), depth_of_field=d, dof_kw=dict(max_coc=K))
    assert capi.image_read_pfm(prefix + "_den.pfm").tobytes() == one["denoised"].tobytes()
    assert capi.image_read_pfm(prefix + "_dof.pfm").tobytes() == one["defocused"].tobytes()
    assert capi.image_read_pfm1(prefix + "_coc.pfm").tobytes() == one["coc"].tobytes()
    assert one["defocused"].tobytes() != one["denoised"].tobytes()


# e_post / e_pin measured on an MI355X: MEASURED_RATIO (with e_noise / e_pin MEASURED_NOISE); the bound is halfway from there to 1
MEASURED_RATIO, MEASURED_NOISE = 0.664, 0.472
LENS_BOUND = 0.5 * (MEASURED_RATIO + 1.0)


def lens_errors(w=96, h=72, spp=256):
    """(e_noise, e_pin, e_post, A): RMSEs in linear colour against the renderer's own lens render L of cornell.xml -- of a second
    lens render with another seed, of the pinhole render P, and of the stage applied to P"""
    s, cam = _lens_camera(w, h)
    s.set_render_flags(capi.RENDER_REPRODUCIBLE)                # the same figures on every run
    pin = capi._copy_camera(cam)
    pin.dof = 0.0
    L1 = s.render_outputs(cam, _params(21, spp), planes=("linear",))["linear"]
    L2 = s.render_outputs(cam, _params(22, spp), planes=("linear",))["linear"]
    P = s.render_outputs(pin, _params(21, spp), planes=("linear",))
    with capi.DepthOfField(0, w, h) as d:
        S = d.apply(P["linear"], P["z"], cam)
    ok = np.isfinite(L1).all(axis=2) & np.isfinite(L2).all(axis=2) & np.isfinite(P["linear"]).all(axis=2) & np.isfinite(S).all(axis=2)
    rmse = lambda a, b: float(np.sqrt(np.mean((a[ok].astype(np.float64) - b[ok].astype(np.float64)) ** 2)))
    return rmse(L1, L2), rmse(P["linear"], L1), rmse(S, L1), float(ref_setup(cam)[0])


@pytest.mark.gpu
def test_stage_against_the_lens_render():
    e_noise, e_pin, e_post, A = lens_errors()
    print(f"dof against the lens render: A {A:.2f} px, e_noise {e_noise:.5f}, e_pin {e_pin:.5f}, e_post {e_post:.5f}, "
          f"e_post / e_pin {e_post / e_pin:.3f}, e_noise / e_pin {e_noise / e_pin:.3f}")
    assert 5.0 < A < 7.0
    assert e_pin > 2 * e_noise                                  # the scene shows the effect at all
    assert e_post < e_pin
    assert e_post / e_pin < LENS_BOUND
