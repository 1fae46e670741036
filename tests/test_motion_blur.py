"""Motion blur (include/rt_mi355x.h, "motion blur"): rt_motion_blur_*, capi.MotionBlur, Scene.render_temporal(motion_blur=), the
C++ shim's EnableMotionBlur().

ref_motion_blur is a numpy transcription of the definition.  Its discrete decisions -- v, m, both selections, the clamp factor, the
early out and the tap pixels -- are float32 in the stated order whatever `dtype` is; the weights and the colour sums are taken in
`dtype`.  float64 is the yardstick; with float32 numpy rounds every operation on its own, which is what a device does, and the gate
is held against that evaluation too, on the CPU.  out_tiles and the pixels that pass through are compared bit for bit.

Gate: C * 2^-24 * max(|c| over the centre and the pixel's live taps) + 1e-7, C counted in roundings (u = 2^-24 each).  The output is a
normalised average, out = S / W with S = sum w_k c_k, so an ABSOLUTE error dw_k of a weight moves it by dw_k (c_k - out) / W, at most
2 max|c| dw_k / W: cone, near and the smoothstep subtract, so their errors are absolute, and how much they matter depends on W.
  t_i      a_i is exact; a_i * g (below 2): 2u; - 1: u.  dt <= 3u.
  L, l     one sqrt each: relative u.
  d        |t| L: L dt + |t| dL + u d <= 5u L.
  cone     q = d / l: dd / l + q (u + u); 1 - q: u.  Where q > 1 both sides clamp to 0: 5u L / l + 3u.
  cyl      e0, e1 = 0.95 l, 1.05 l: 1.9u l, 2.1u l; e1 - e0 (0.1 l): 4.1u l, relative 41u.  d - e0 inside the ramp (at most 0.1 l):
           5u L + 2u l.  T: (5u L + 2u l) / (0.1 l) + 42u = 50u L / l + 62u.  The smoothstep's slope is at most 1.5: 75u L / l + 93u;
           its own products and the 3 - 2 T: 3u; 1 - that: u.  75u L / l + 97u.
  near     e: u; a - b: u; the quotient (inside the ramp at most 1): 3u; 1 - r (at most 2): 2u.  5u.
  w        near * cone: 5u L / l + 9u each, their sum 2u; cyl * cyl: 75u L (1 / ls + 1 / lp) + 195u, doubled; the last sum (w <= 4): 4u.
           dw <= u (155 L (1 / ls + 1 / lp) + 414), taken as A = 155 L (1 / ls + 1 / lp) + 420.
  centre   w_p = 1 / lp: 2u relative, 4u of max|c| at most.
  sums     n <= N + 1 terms: the products and additions of S n u, those of W (n - 1) u, the division u: below (2 N + 2) u max|c|.
  C = 2 N + 8 + 2 sum_i A_i / W, per pixel, from the float64 evaluation's L, ls, lp and W.  With L <= K, l >= 0.5 and W >= 1 / K a
  closed bound is 2 N + 8 + 2 N K (620 K + 420), which is of no use as a gate at K = 32; hence the count per pixel."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from raytracing_folder_amd import capi
from tests import scenes
from tests.stage_support import (F, SPHERE_CHILD, SPHERE_STEP, U, assert_driver_usage, build_driver, move_sphere as _move_sphere,
                                 sphere_params as _sphere_params)

DEFAULTS = dict(shutter=0.5, max_blur=16, samples=15, depth_extent=0.05)
JITTER = (0, 2, 3, 1)
FAR = F(1e30)


# ---- the transcription --------------------------------------------------------------------------------------------
def ref_velocity(motion, shutter):
    """step 1: (vx, vy, m), float32 (H, W) each"""
    motion = np.asarray(motion, F)
    H, W = motion.shape[:2]
    Y, X = np.mgrid[0:H, 0:W]
    h = F(0.5) * F(shutter)
    fx, fy, ze = motion[..., 0], motion[..., 1], motion[..., 2]
    with np.errstate(all="ignore"):
        ok = (ze > 0) & np.isfinite(fx) & np.isfinite(fy) & np.isfinite(ze)
        vx = np.where(ok, h * (X.astype(F) - fx), F(0)).astype(F)
        vy = np.where(ok, h * (Y.astype(F) - fy), F(0)).astype(F)
        return vx, vy, (vx * vx + vy * vy).astype(F)


def ref_tiles(vx, vy, m, K):
    """steps 2 and 3: the unclamped neighbour-max vector per tile, float32 (TY, TX, 2)"""
    H, W = m.shape
    TX, TY = -(-W // K), -(-H // K)
    pad = np.full((TY * K, TX * K), F(-1))
    pad[:H, :W] = m
    k = pad.reshape(TY, K, TX, K).transpose(0, 2, 1, 3).reshape(TY, TX, K * K).argmax(axis=2)     # the first of equals: the lowest index
    py, px = np.arange(TY)[:, None] * K + k // K, np.arange(TX)[None, :] * K + k % K
    tx, ty = vx[py, px], vy[py, px]
    with np.errstate(all="ignore"):
        tm = (tx * tx + ty * ty).astype(F)
    bm, bx, by = np.full((TY, TX), F(-1)), np.zeros((TY, TX), F), np.zeros((TY, TX), F)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            sm, sx, sy = np.full((TY, TX), F(-2)), np.zeros((TY, TX), F), np.zeros((TY, TX), F)
            ys, xs = slice(max(0, -dy), TY - max(0, dy)), slice(max(0, -dx), TX - max(0, dx))
            yn, xn = slice(ys.start + dy, ys.stop + dy), slice(xs.start + dx, xs.stop + dx)
            sm[ys, xs], sx[ys, xs], sy[ys, xs] = tm[yn, xn], tx[yn, xn], ty[yn, xn]
            take = sm > bm
            bm, bx, by = np.where(take, sm, bm), np.where(take, sx, bx), np.where(take, sy, by)
    return np.stack([bx, by], axis=2).astype(F)


def ref_motion_blur(rgb, motion, z, dtype=np.float64, jitter=JITTER, **kw):
    """the definition: (out in `dtype`, out_tiles float32 (TY, TX, 2), the pixels that pass through unchanged, C of the gate per
    pixel, max|c| over the centre and the live taps per pixel)"""
    p = dict(DEFAULTS, **kw)
    K, N = int(p["max_blur"]), int(p["samples"])
    dt = dtype
    c_ = lambda v: dt(F(v))                                     # a float constant of the definition
    rgb, z = np.asarray(rgb, F), np.asarray(z, F)
    H, W = z.shape
    Y, X = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        vx, vy, m = ref_velocity(motion, p["shutter"])
        tiles = ref_tiles(vx, vy, m, K)
        nx, ny = tiles[Y // K, X // K, 0], tiles[Y // K, X // K, 1]
        mn = (nx * nx + ny * ny).astype(F)
        early = mn < F(0.25)
        fin_p = np.isfinite(rgb).all(axis=2)
        big = ~(mn <= F(K * K))
        f = F(K) / np.sqrt(mn)
        cx, cy = np.where(big, nx * f, nx).astype(F), np.where(big, ny * f, ny).astype(F)
        lenK = lambda mm: np.minimum(np.sqrt(mm.astype(dt)), dt(K))
        clamp01 = lambda a: np.minimum(np.maximum(a, dt(0)), dt(1))
        cone = lambda d, l: clamp01(dt(1) - d / l)

        def cyl(d, l):
            e0, e1 = c_(0.95) * l, c_(1.05) * l
            u = clamp01((d - e0) / (e1 - e0))
            return dt(1) - (u * u) * (dt(3) - dt(2) * u)

        def near(a, b):
            e = c_(p["depth_extent"]) * np.maximum(np.minimum(a, b), c_(1e-6))
            return clamp01(dt(1) - (a - b) / e)

        L = lenK(mn)
        lp = np.maximum(lenK(m), dt(0.5))
        zz = np.where(np.isfinite(z) & (z < FAR), z, FAR).astype(dt)
        wp = dt(1) / lp
        Wsum = wp.copy()
        S = wp[..., None] * np.where(fin_p[..., None], rgb, F(0)).astype(dt)
        A = np.zeros((H, W))
        maxc = np.abs(np.where(fin_p[..., None], rgb, F(0))).max(axis=2).astype(np.float64)
        j = np.asarray(jitter)[(Y & 1) * 2 + (X & 1)]
        joff = F(0.125) + F(0.25) * j.astype(F)
        g = F(2) / F(N)
        for i in range(N):
            a = (F(i) + joff).astype(F)
            t32 = (a * g - F(1)).astype(F)
            sxf = np.floor((X.astype(F) + t32 * cx) + F(0.5))
            syf = np.floor((Y.astype(F) + t32 * cy) + F(0.5))
            inside = (sxf >= 0) & (sxf < W) & (syf >= 0) & (syf < H)
            sx, sy = np.where(inside, sxf, 0).astype(np.int64), np.where(inside, syf, 0).astype(np.int64)
            cs = rgb[sy, sx]
            live = inside & np.isfinite(cs).all(axis=2)
            cs = np.where(live[..., None], cs, F(0))
            t = a.astype(dt) * dt(g) - dt(1)
            d = np.abs(t) * L
            ls = np.maximum(lenK(m[sy, sx]), dt(0.5))
            zs = zz[sy, sx]
            w = (near(zs, zz) * cone(d, ls) + near(zz, zs) * cone(d, lp)) + dt(2) * (cyl(d, ls) * cyl(d, lp))
            w = np.where(live, w, dt(0)).astype(dt)
            Wsum = Wsum + w
            S = S + w[..., None] * cs.astype(dt)
            A += np.where(live, 155.0 * L * (1.0 / ls + 1.0 / lp) + 420.0, 0.0)
            maxc = np.maximum(maxc, np.abs(cs).max(axis=2))
        out = S / Wsum[..., None]
        through = early | ~fin_p
        out = np.where(through[..., None], rgb.astype(dt), out)
        Cp = 2 * N + 8 + 2.0 * A / Wsum.astype(np.float64)
        return out, tiles, through, Cp, maxc


def over_gate(got, ref):
    """worst error / gate of a blurred plane against a float64 evaluation `ref`; the pixels that pass through must hold the same
    bytes"""
    want, _, through, Cp, maxc = ref
    got = np.asarray(got)
    assert got[through].astype(F).tobytes() == want[through].astype(F).tobytes()
    gate = (Cp * U * maxc + 1e-7)[..., None]
    with np.errstate(invalid="ignore"):                         # the pixels that pass through may hold a NaN or an inf
        err = np.abs(got.astype(np.float64) - want)[~through]
    assert np.isfinite(want[~through]).all() and np.isfinite(got[~through]).all()
    return float((err / np.broadcast_to(gate, want.shape)[~through]).max()) if err.size else 0.0


# ---- the frames -------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 7), (5, 40), (37, 23), (64, 64), (130, 66)]
KS = (2, 8, 16, 32)
KINDS = ("static", "t0.4", "t3", "t1.5K", "square_near", "square_far", "random", "edge")
H_DEFAULT = F(0.25)                                             # 0.5f * the default shutter


def colours(w, h, seed=1):
    rng = np.random.default_rng(seed)
    Y = 2.0 ** rng.uniform(-4.0, 4.0, (h, w))
    return (Y[..., None] * rng.uniform(0.5, 1.5, (h, w, 3))).astype(F)


def moved(w, h, vx, vy, z):
    """the motion plane whose pixels have the velocity (vx, vy) at the default shutter, as far as float allows: fx = x - vx / h"""
    Y, X = np.mgrid[0:h, 0:w]
    vx, vy = np.broadcast_to(np.asarray(vx, F), (h, w)), np.broadcast_to(np.asarray(vy, F), (h, w))
    return np.stack([X.astype(F) - vx / H_DEFAULT, Y.astype(F) - vy / H_DEFAULT, np.asarray(z, F)], axis=2).astype(F)


def frame(w, h, K, kind, seed=1):
    """(rgb, motion, z) float32.  The translations are named by the length of v, the blur's half extent in pixels: 0.4 is under the
    early out, 3 is gathered, 1.5 K is clamped."""
    rng = np.random.default_rng(seed + 7)
    rgb = colours(w, h, seed)
    z = rng.uniform(1.0, 20.0, (h, w)).astype(F)
    if kind == "static":
        return rgb, moved(w, h, 0.0, 0.0, z), z
    if kind in ("t0.4", "t3", "t1.5K"):
        s = {"t0.4": 0.4, "t3": 3.0, "t1.5K": 1.5 * K}[kind]
        return rgb, moved(w, h, 0.8 * s, -0.6 * s, z), z
    if kind in ("square_near", "square_far"):
        sq = np.zeros((h, w), bool)
        sq[h // 4:h // 4 + max(1, h // 3), w // 4:w // 4 + max(1, w // 3)] = True
        fast = sq if kind == "square_near" else ~sq
        z = np.where(sq, F(5.0), F(10.0)).astype(F)
        return rgb, moved(w, h, np.where(fast, F(0.9 * K), F(0)), np.where(fast, F(0.3 * K), F(0)), z), z
    if kind == "edge":                                          # static but for one pixel at m = 0.25 exactly and one just under it
        mv = moved(w, h, 0.0, 0.0, z)
        if w * h >= 64:
            mv[h // 4, w // 4, 0] -= F(2.0)
            at = (h - 1 - h // 4, w - 1 - w // 4)
            mv[at][0] = np.nextafter(mv[at][0] - F(2.0), F(np.inf))
        return rgb, mv, z
    assert kind == "random"
    mag = 10.0 ** rng.uniform(-2.0, 2.0, (h, w))
    ang = rng.uniform(0.0, 2.0 * np.pi, (h, w))
    mv = moved(w, h, mag * np.cos(ang), mag * np.sin(ang), z)
    flat_mv, flat_z, flat_c = mv.reshape(-1, 3), z.reshape(-1), rgb.reshape(-1, 3)
    X = np.arange(w * h) % w
    if w >= 2:                                                  # two pixels of the first tile with equal m, different directions
        flat_mv[0, :2] = (X[0] - 512.0, 0.0)
        flat_mv[1, :2] = (X[1], 0.0 - 512.0)
    far = (w - 1 - K, h - 1) if w - 1 - K >= 0 else ((w - 1, h - 1 - K) if h - 1 - K >= 0 else None)
    if far is not None and w * h >= 64:                         # the same tie across two neighbouring tiles
        mv[h - 1, w - 1, :2] = (w - 1 + 1024.0, h - 1)
        mv[far[1], far[0], :2] = (far[0], far[1] + 1024.0)
    if w * h >= 64:
        at = w * (h // 2) + w // 2
        flat_mv[at, 2] = 0.0                                    # no previous position
        flat_mv[at + 1, 0] = np.nan
        flat_z[at + 2] = 1e30
        flat_z[at + 3] = np.inf
        flat_mv[at + 4, :2] = (X[at + 4] - 2.0, (at + 4) // w)              # m = 0.25 exactly
        flat_mv[at + 5, :2] = (X[at + 5] - 4.0 * K, (at + 5) // w)          # m = K^2 exactly
        flat_c[at + 6] = (np.nan, 1.0, 1.0)
        flat_c[at + 7] = (1.0, np.inf, 1.0)
        flat_mv[at - 1, 1] = np.inf
        flat_mv[at - 2, 2] = -3.0
    return rgb, mv, z


def cases(size):
    """(K, N, kind) of the comparisons at one size: every kind at N = 15, the two with the most going on at N = 3 as well"""
    return [(K, N, kind) for K in KS for kind in KINDS for N in ((15, 3) if kind in ("random", "square_near") else (15,))]


_REF = {}


def reference(w, h, K, N, kind, dtype=np.float64):
    """the transcription of frame(w, h, K, kind) at the default shutter and depth extent, computed once and shared"""
    key = (w, h, K, N, kind, dtype)
    if key not in _REF:
        _REF[key] = ref_motion_blur(*frame(w, h, K, kind), dtype=dtype, max_blur=K, samples=N)
    return _REF[key]


# ---- without a GPU -------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("rt_motion_blur_create", "rt_motion_blur_destroy", "rt_motion_blur_default_params", "rt_motion_blur_tiles",
               "rt_motion_blur_device", "rt_motion_blur_host")


def test_new_symbols_struct_layout_and_defaults():
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert L.rt_abi_version() == 4
    assert [f[0] for f in capi.MotionBlurParams._fields_] == ["struct_size", "shutter", "max_blur", "samples", "depth_extent"]
    assert [f[0] for f in capi.MotionBlurPlanes._fields_] == ["struct_size", "rgb_linear", "motion", "z", "out", "out_tiles"]
    assert C.sizeof(capi.MotionBlurParams) == 20 and C.sizeof(capi.MotionBlurPlanes) == 48
    p = capi.MotionBlurParams()
    L.rt_motion_blur_default_params(C.byref(p))
    assert p.struct_size == 20
    for k, v in DEFAULTS.items():
        assert getattr(p, k) == (v if k in ("max_blur", "samples") else F(v)), k
    L.rt_motion_blur_default_params(None)                       # ignored
    L.rt_motion_blur_destroy(None)                              # ignored
    with pytest.raises(TypeError):
        capi.motion_blur_params(gamma=2.2)
    assert capi.motion_blur_params(samples=3, shutter=1.0).samples == 3
    # the existing structs did not grow
    assert C.sizeof(capi.ToneMapParams) == 52 and C.sizeof(capi.ToneMapPlanes) == 40 and C.sizeof(capi.Outputs) == 72
    assert C.sizeof(capi.BloomParams) == 28 and C.sizeof(capi.BloomPlanes) == 32


def test_tiles_equal_ceil():
    for w, h in SIZES + [(1920, 1080), (1, 4096), (7, 1)]:
        for K in (2, 3, 5, 8, 16, 31, 32):
            assert capi.motion_blur_tiles(w, h, K) == (math.ceil(w / K), math.ceil(h / K)), (w, h, K)
    assert capi.motion_blur_tiles(1920, 1080) == (120, 68)
    L = capi.lib()
    assert L.rt_motion_blur_tiles(0, 4, 16, None, None) == -1 and b"bad image size" in L.rt_last_error()
    for bad in (1, 33, 0, -2):
        assert L.rt_motion_blur_tiles(4, 4, bad, None, None) == -1 and b"max_blur" in L.rt_last_error()
    assert L.rt_motion_blur_tiles(4, 4, 2, None, None) == 0


def _arg_cases():
    n = 8 * 8
    buf = np.zeros(n * 3 * 3 + n + 64, np.float32)
    ptr = buf.ctypes.data
    full = lambda **kw: capi.MotionBlurPlanes(**{**dict(rgb_linear=ptr, motion=ptr + n * 12, z=ptr + n * 24, out=ptr + n * 28,
                                                        out_tiles=ptr + n * 40), **kw})
    nan, inf = float("nan"), float("inf")
    cases_ = []
    for bad in (0, 19, 24):
        p = capi.motion_blur_params()
        p.struct_size = bad
        cases_.append((b"struct_size", p, full()))
    pl = full()
    pl.struct_size += 8
    cases_.append((b"struct_size", capi.motion_blur_params(), pl))
    for bad in (-0.5, 2.5, nan, inf):
        cases_.append((b"shutter", capi.motion_blur_params(shutter=bad), full()))
    for bad in (1, 0, 33, -4):
        cases_.append((b"max_blur is", capi.motion_blur_params(max_blur=bad), full()))
    for bad in (1, 2, 4, 14, 64, 65, -3):
        cases_.append((b"samples is", capi.motion_blur_params(samples=bad), full()))
    for bad in (0.0, 5e-4, -1.0, nan, inf):
        cases_.append((b"depth_extent", capi.motion_blur_params(depth_extent=bad), full()))
    for name in ("rgb_linear", "motion", "z", "out"):
        cases_.append((b"are required", capi.motion_blur_params(), full(**{name: None})))
    return buf, cases_, full


def test_argument_checks_come_before_any_gpu_call():
    """every check that does not need the object is reached with a NULL one, so it is reached without a device; the one that does
    (overlapping planes: the size is the object's) is in test_argument_checks_with_an_object"""
    L = capi.lib()
    buf, cases_, full = _arg_cases()
    for what, p, pl in cases_:
        for st in (L.rt_motion_blur_host(None, C.byref(p), C.byref(pl)), L.rt_motion_blur_device(None, None, C.byref(p), C.byref(pl), 1)):
            assert st == -1 and what in L.rt_last_error(), (what, L.rt_last_error())
    p, pl = capi.motion_blur_params(), full()
    for args in ((None, C.byref(pl)), (C.byref(p), None)):
        assert L.rt_motion_blur_host(None, *args) == -1 and L.rt_motion_blur_device(None, None, *args, 1) == -1
    assert L.rt_motion_blur_host(None, C.byref(p), C.byref(pl)) == -1 and b"rt_motion_blur is NULL" in L.rt_last_error()
    for ok in (dict(shutter=0.0), dict(shutter=2.0), dict(max_blur=2), dict(max_blur=32), dict(samples=3), dict(samples=63), dict(depth_extent=1e-3)):
        q = capi.motion_blur_params(**ok)                       # the ends of the ranges pass every check up to the object
        assert L.rt_motion_blur_host(None, C.byref(q), C.byref(pl)) == -1 and b"rt_motion_blur is NULL" in L.rt_last_error(), ok
    h = C.c_void_p()
    for w_, h_ in ((0, 8), (8, 0), (-3, 8)):
        assert L.rt_motion_blur_create(0, w_, h_, C.byref(h)) == -1 and b"bad image size" in L.rt_last_error() and not h
    assert L.rt_motion_blur_create(0, 8, 8, None) == -1
    # more than 2^30 pixels: RT_ERR_LIMIT, after the argument checks and before the device is looked for
    assert L.rt_motion_blur_create(0, 1 << 16, (1 << 14) + 1, C.byref(h)) == -6 and b"2^30" in L.rt_last_error() and not h
    if capi.device_count() == 0:                                # ... and RT_ERR_NO_DEVICE comes after all of them
        assert L.rt_motion_blur_create(0, 8, 8, C.byref(h)) == -3 and not h
        with pytest.raises(capi.RtError) as err:
            capi.MotionBlur(0, 8, 8)
        assert err.value.status == -3


def test_shim_driver_builds_against_the_header(tmp_path):
    assert_driver_usage(build_driver(tmp_path, "shim_motion_blur_driver"))


def test_frames_hold_what_the_tests_rely_on():
    K = 8
    for kind, lo, hi in (("t0.4", 0.39, 0.41), ("t3", 2.99, 3.01), ("t1.5K", 11.9, 12.1)):
        _, mv, _ = frame(37, 23, K, kind)
        m = ref_velocity(mv, 0.5)[2]
        assert lo ** 2 < m.min() and m.max() < hi ** 2, kind
    rgb, mv, z = frame(37, 23, K, "random")
    vx, vy, m = ref_velocity(mv, 0.5)
    assert (m == F(0.25)).sum() == 1 and (m == F(K * K)).sum() == 1
    assert m[0, 0] == m[0, 1] == F(128.0 ** 2) and (vx[0, 0], vy[0, 1]) == (128.0, 128.0)       # a tie inside the first tile
    assert m[22, 36] == m[22, 36 - K] == F(256.0 ** 2) and vx[22, 36] != vx[22, 36 - K]           # ... and across two tiles
    assert m[m > 0].min() < 1e-3 and np.sort(m.ravel())[-5] > 50.0 ** 2
    assert (~np.isfinite(mv)).any(axis=2).sum() == 2 and (mv[..., 2] <= 0).sum() == 2 and (m == 0).sum() == 4
    assert np.isinf(z).sum() == 1 and (z == FAR).sum() == 1 and (~np.isfinite(rgb)).any(axis=2).sum() == 2
    tiles = ref_tiles(vx, vy, m, K)
    assert tuple(tiles[0, 0]) == (128.0, 0.0)                   # the lower index of the tie won
    _, mv, _ = frame(37, 23, K, "edge")
    through = ref_motion_blur(*frame(37, 23, K, "edge"), max_blur=K)[2]
    m = ref_velocity(mv, 0.5)[2]
    assert (m == F(0.25)).sum() == 1 and ((m > 0) & (m < F(0.25))).sum() == 1
    assert not through[23 // 4, 37 // 4] and through[23 - 1 - 23 // 4, 37 - 1 - 37 // 4] and 0 < (~through).sum() < through.sum()


def test_reference_static_and_under_the_early_out_return_the_input():
    for w, h in SIZES:
        for kind in ("static", "t0.4"):
            rgb, mv, z = frame(w, h, 8, kind)
            for dt in (np.float32, np.float64):
                out, tiles, through, _, _ = ref_motion_blur(rgb, mv, z, dt, max_blur=8)
                assert through.all() and out.astype(F).tobytes() == rgb.tobytes()
            assert (tiles == 0).all() == (kind == "static")


def test_reference_keeps_a_constant_colour_under_random_motion():
    for w, h, K in ((37, 23, 8), (64, 64, 16), (130, 66, 32)):
        _, mv, z = frame(w, h, K, "random")
        rgb = np.broadcast_to(np.array([3.0, 0.5, 0.125], F), (h, w, 3)).copy()
        out, _, through, _, _ = ref_motion_blur(rgb, mv, z, max_blur=K)
        assert not through.all()
        assert (np.abs(out - rgb) <= 64 * 2.0 ** -53 * rgb).all()
        out32 = ref_motion_blur(rgb, mv, z, np.float32, max_blur=K, samples=63)[0]
        assert (np.abs(out32 - rgb) <= (2 * 63 + 8) * U * rgb).all()


def test_reference_flipped_left_to_right():
    """frame and motion flipped left to right, on an even width and whole tiles, with the jitter's own flip: a pixel's mirror image
    has the other column parity, so the table is read with that bit swapped.  A uniform translation whose plane is exact in float
    (v = (2.25, 1)), so that every pixel has the one velocity and which pixel a tile picks does not matter; no tap of it falls on
    a pixel boundary."""
    w, h, K = 64, 48, 8
    rgb, z = colours(w, h), np.random.default_rng(5).uniform(1.0, 20.0, (h, w)).astype(F)
    out = ref_motion_blur(rgb, moved(w, h, 2.25, 1.0, z), z, max_blur=K)
    flipped_jitter = tuple(JITTER[i ^ 1] for i in range(4))
    assert flipped_jitter == (2, 0, 1, 3)
    mirror = ref_motion_blur(rgb[:, ::-1], moved(w, h, -2.25, 1.0, z[:, ::-1]), z[:, ::-1], max_blur=K, jitter=flipped_jitter)
    assert not out[2].any() and over_gate(mirror[0][:, ::-1], out) <= 1.0
    assert np.abs(out[0] - rgb).max() > 0.1


def test_reference_nan_pixel_stays_and_changes_no_other():
    rgb, mv, z = frame(37, 23, 8, "random")
    bad = ~np.isfinite(rgb).all(axis=2)
    assert bad.sum() == 2
    other = rgb.copy()
    other[bad] = (np.inf, -np.inf, np.nan)
    a, b = ref_motion_blur(rgb, mv, z, max_blur=8)[0], ref_motion_blur(other, mv, z, max_blur=8)[0]
    assert a[bad].astype(F).tobytes() == rgb[bad].tobytes() and np.isfinite(a[~bad]).all()
    assert a[~bad].tobytes() == b[~bad].tobytes()               # what the bad pixel holds reaches no other pixel


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_counted_gate_holds_for_a_float32_evaluation(size):
    w, h = size
    worst = 0.0
    for K, N, kind in cases(size):
        want, got = reference(w, h, K, N, kind), ref_motion_blur(*frame(w, h, K, kind), dtype=np.float32, max_blur=K, samples=N)
        assert got[1].tobytes() == want[1].tobytes() and (got[2] == want[2]).all()
        worst = max(worst, over_gate(got[0], want))
    print(f"motion blur float32 evaluation {w}x{h}: worst error / gate {worst:.3f}")
    assert worst <= 1.0


# ---- on the GPU ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_against_the_float64_transcription(size):
    w, h = size
    worst = 0.0
    with capi.MotionBlur(0, w, h) as mb:
        for K, N, kind in cases(size):
            rgb, mv, z = frame(w, h, K, kind)
            keep = [a.copy() for a in (rgb, mv, z)]
            out, tiles = mb.apply(rgb, mv, z, return_tiles=True, max_blur=K, samples=N)
            ref = reference(w, h, K, N, kind)
            assert tiles.tobytes() == ref[1].tobytes(), (K, N, kind)
            worst = max(worst, over_gate(out, ref))
            if kind in ("static", "t0.4"):
                assert out.tobytes() == rgb.tobytes(), (K, kind)
            for a, b in zip(keep, (rgb, mv, z)):
                assert a.tobytes() == b.tobytes()
    print(f"motion blur {w}x{h}: worst error / gate {worst:.3f}")
    assert worst <= 1.0


# (w, h, K) at the edges of the tile-gather geometry (csrc/rt_tile_gather.h; G = the tiles along a gather workgroup's square):
# the smallest image; narrower than one tile, one tile column, G = 1; G = 8 with a ragged last square and tile in x and one tile
# row; G = 3, a square of 15 pixels, ragged in both axes; the first K with G = 1, one workgroup of 81 pixels; everything divides;
# one pixel over in both axes
GEOMETRY = [(1, 1, 2), (3, 70, 32), (70, 3, 2), (33, 17, 5), (31, 33, 9), (64, 48, 8), (65, 49, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", GEOMETRY, ids=lambda s: f"{s[0]}x{s[1]}-K{s[2]}")
def test_device_at_the_edges_of_the_tile_geometry(shape):
    w, h, K = shape
    worst = 0.0
    with capi.MotionBlur(0, w, h) as mb:
        for kind in ("random", "square_near"):
            rgb, mv, z = frame(w, h, K, kind)
            out, tiles = mb.apply(rgb, mv, z, return_tiles=True, max_blur=K, samples=15)
            ref = reference(w, h, K, 15, kind)
            assert tiles.shape == ref[1].shape and tiles.tobytes() == ref[1].tobytes(), kind
            worst = max(worst, over_gate(out, ref))
    print(f"motion blur {w}x{h} K {K}: worst error / gate {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.gpu
def test_exact_properties_on_the_device():
    import torch
    w, h, K = 37, 23, 8
    rgb, mv, z = frame(w, h, K, "random")
    tx, ty = capi.motion_blur_tiles(w, h, K)
    with capi.MotionBlur(0, w, h) as mb:
        first, again = mb.apply(rgb, mv, z, return_tiles=True, max_blur=K), mb.apply(rgb, mv, z, return_tiles=True, max_blur=K)
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
        assert mb.apply(rgb, mv, z, max_blur=K).tobytes() == first[0].tobytes()
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(device=dev)
        src, mot, dep = (torch.from_numpy(a).to(dev) for a in (rgb, mv, z))
        out, out2 = torch.zeros_like(src), torch.zeros_like(src)
        tiles = torch.zeros((ty, tx, 2), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        ptrs = dict(linear_ptr=src.data_ptr(), motion_ptr=mot.data_ptr(), z_ptr=dep.data_ptr())
        mb.apply_device(side.cuda_stream, out_ptr=out.data_ptr(), tiles_ptr=tiles.data_ptr(), max_blur=K, **ptrs)
        mb.apply_device(side.cuda_stream, out_ptr=out2.data_ptr(), sync=True, max_blur=K, **ptrs)
        assert out.cpu().numpy().tobytes() == first[0].tobytes() == out2.cpu().numpy().tobytes()
        assert tiles.cpu().numpy().tobytes() == first[1].tobytes()
        for t, a in ((src, rgb), (mot, mv), (dep, z)):          # the source planes are as they were
            assert t.cpu().numpy().tobytes() == a.tobytes()
        # a constant colour is kept, whatever the motion
        flat = np.broadcast_to(np.array([3.0, 0.5, 0.125], F), (h, w, 3)).copy()
        got = mb.apply(flat, mv, z, max_blur=K, samples=63)
        assert (np.abs(got - flat) <= (2 * 63 + 8) * U * flat).all() and (got != flat).any()
        # shutter 0: nothing moves
        assert mb.apply(rgb, mv, z, max_blur=K, shutter=0.0).tobytes() == rgb.tobytes()


@pytest.mark.gpu
def test_argument_checks_with_an_object():
    import torch
    L = capi.lib()
    n = 8 * 8
    t = torch.zeros((n * 12,), dtype=torch.float32, device="cuda:0")
    ptr = t.data_ptr()
    p = capi.motion_blur_params(max_blur=2)                     # 4 x 4 tiles: out_tiles is 128 bytes
    good = dict(rgb_linear=ptr, motion=ptr + n * 12, z=ptr + n * 24, out=ptr + n * 28, out_tiles=ptr + n * 40)
    with capi.MotionBlur(0, 8, 8) as mb:
        _, cases_, _ = _arg_cases()
        for what, bad, pl in cases_:                            # the same refusals with an object
            assert L.rt_motion_blur_host(mb._h, C.byref(bad), C.byref(pl)) == -1 and what in L.rt_last_error(), what
        for over in (dict(out=ptr), dict(out=ptr + 12), dict(out=ptr + n * 12 - 4), dict(out=ptr + n * 24), dict(motion=ptr + n * 12 - 4),
                     dict(z=ptr), dict(out_tiles=ptr + n * 28 + n * 12 - 4), dict(out_tiles=ptr + n * 12 - 124)):
            pl = capi.MotionBlurPlanes(**dict(good, **over))
            assert L.rt_motion_blur_device(mb._h, None, C.byref(p), C.byref(pl), 1) == -1 and b"overlap" in L.rt_last_error(), over
        assert L.rt_motion_blur_device(mb._h, None, C.byref(p), C.byref(capi.MotionBlurPlanes(**good)), 1) == 0
        assert L.rt_motion_blur_device(mb._h, None, C.byref(p), C.byref(capi.MotionBlurPlanes(**dict(good, out_tiles=None))), 1) == 0


@pytest.mark.gpu
def test_render_temporal_with_a_motion_blur():
    """cornell.xml at 96 x 72 with sphere1 moved between two frames, reproducible mode"""
    w, h, K = 96, 72, 8
    kw = dict(shutter=1.0, max_blur=K)
    s, cam = scenes.load_cornell(w, h)
    s.set_render_flags(capi.RENDER_REPRODUCIBLE)
    with capi.MotionBlur(0, w, h) as mb, capi.Bloom(0, w, h) as bl, capi.Exposure(0) as exp, \
            capi.History(0, w, h) as hst, capi.History(0, w, h) as hst_plain:
        with pytest.raises(ValueError):
            s.render_temporal(hst, cam, _sphere_params(11), motion_blur=mb)
        assert hst.frames == 0
        one = s.render_temporal(hst, cam, _sphere_params(11), moving=True, motion_blur=mb, motion_blur_kw=kw)
        plain = s.render_temporal(hst_plain, cam, _sphere_params(11), moving=True)
        assert set(one) == set(plain) | {"motion_blurred"}
        for k, v in plain.items():
            if isinstance(v, np.ndarray):
                assert one[k].tobytes() == v.tobytes(), k
        assert one["motion_blurred"].tobytes() == one["denoised"].tobytes()     # nothing has moved yet
        idx = _move_sphere(s)[0]
        two = s.render_temporal(hst, cam, _sphere_params(12), moving=True, motion_blur=mb, motion_blur_kw=kw, bloom=bl, exposure=exp)
        plain = s.render_temporal(hst_plain, cam, _sphere_params(12), moving=True)
        assert set(two) == set(plain) | {"motion_blurred", "bloomed", "display_rgb"}
        for k, v in plain.items():
            if isinstance(v, np.ndarray):
                assert two[k].tobytes() == v.tobytes(), k
        blurred, tiles = mb.apply(two["denoised"], two["motion"], two["z"], return_tiles=True, **kw)
        assert two["motion_blurred"].tobytes() == blurred.tobytes()
        assert two["bloomed"].tobytes() == bl.apply(blurred).tobytes()          # exp held no metered frame when the frame was bloomed
        # every pixel whose 3 x 3 tile neighbourhood is at rest is the input's; around the moved sphere something changed
        m = ref_velocity(two["motion"], kw["shutter"])[2]
        ref_t = ref_tiles(*ref_velocity(two["motion"], kw["shutter"]), K)
        assert tiles.tobytes() == ref_t.tobytes()
        Y, X = np.mgrid[0:h, 0:w]
        quiet = ((ref_t ** 2).sum(axis=2) < 0.25)[Y // K, X // K]
        assert quiet.any() and not quiet.all()
        assert blurred[quiet].tobytes() == two["denoised"][quiet].tobytes()
        on = two["object_id"] == idx
        assert on.sum() >= 8 and m[on].max() > 0.25 and (blurred[on] != two["denoised"][on]).any()
        # the accumulated plane when the denoise is off
        three = s.render_temporal(hst, cam, _sphere_params(13), moving=True, denoise=False, motion_blur=mb, motion_blur_kw=kw)
        assert "denoised" not in three
        assert three["motion_blurred"].tobytes() == mb.apply(three["accumulated"], three["motion"], three["z"], **kw).tobytes()


@pytest.mark.gpu
def test_cpp_shim_motion_blur_equals_the_capi_one(tmp_path):
    exe = build_driver(tmp_path, "shim_motion_blur_driver")
    prefix = str(tmp_path / "f")
    w, h = 64, 48
    r = subprocess.run([exe, scenes.CORNELL, prefix, str(w), str(h), str(SPHERE_CHILD)] + [str(v) for v in SPHERE_STEP], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    s, cam = scenes.load_cornell(w, h)
    s.set_render_flags(capi.RENDER_REPRODUCIBLE)
    kw = dict(shutter=1.0, max_blur=8)
    with capi.History(0, w, h) as hst, capi.MotionBlur(0, w, h) as mb:
        one = s.render_temporal(hst, cam, _sphere_params(11), denoise=False, moving=True, motion_blur=mb, motion_blur_kw=kw)
        _move_sphere(s)
        two = s.render_temporal(hst, cam, _sphere_params(12), denoise=False, moving=True, motion_blur=mb, motion_blur_kw=kw)
    assert capi.image_read_pfm(prefix + "_mb1.pfm").tobytes() == one["motion_blurred"].tobytes() == one["accumulated"].tobytes()
    assert capi.image_read_pfm(prefix + "_acc2.pfm").tobytes() == two["accumulated"].tobytes()
    assert capi.image_read_pfm(prefix + "_mb2.pfm").tobytes() == two["motion_blurred"].tobytes()
    assert two["motion_blurred"].tobytes() != two["accumulated"].tobytes()
