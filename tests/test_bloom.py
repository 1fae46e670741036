"""Bloom (include/rt_mi355x.h, "bloom"): rt_bloom_*, capi.Bloom, Scene.render_denoised / render_temporal with bloom=, the C++
shim's EnableBloom().

ref_bloom is a numpy transcription of the definition.  With dtype float64 it is the yardstick (the float32 constants of the
definition, everything else in double); with dtype float32 numpy rounds every product and sum on its own, which is what a device
does -- the counted gate is held against that evaluation too, on the CPU.

Gate: C * 2^-24 * |want| + 1e-7 with C counted in roundings (u = 2^-24 relative each) along the longest chain of the definition:
  bright pass  Y: a product and two sums of non-negative terms, 3.  Ys = scale * Y: 4, and 2 more where the scale is an exp2 taken
               on both sides (the device's double exp2 and numpy's may round to neighbouring floats): 6.
               d = Ys - t is the one subtraction of the stage: its error relative to its RESULT is the error of Ys times Ys / d.
               Above the knee (d >= k) that factor is at most (t + k) / k = 3 for knee 0.5: d 3 * 6 + 1 = 19.  In the knee
               x = d + k, factor Ys / x: where x >= Ys / 3, x: 3 * 6 + 2 = 20; x * x: 41; den = 4 k + 1e-5f: 1; the quotient: 43;
               max(s, d): 43; max(Ys, 1e-5f): 6; wgt: 43 + 6 + 1 = 50; c * wgt: 51.  Deeper in the knee (x < Ys / 3) the
               contribution is c x^2 / (4 k Ys) and its ABSOLUTE error about 12 u c x / (4 k): for the frames here (t = 1,
               k = 0.5, channels at most 3 Ys) at most 27 u x, which the 51 u |want| + 1e-7 of the gate covers for every x in
               (0, 0.25) (it is below 1e-7 up to x = 0.06, and from there the relative part has grown to more than it).
  pyramid      a level down: f horizontally (3 b: 1, a + 3 b: 2, the outer sum: 3; * 0.125 is exact) and vertically: 6.
               a level up: g horizontally (0.75 n: 1, the sum: 2; 0.25 f is exact) and vertically: 4, and the lerp (a: 1, a B: 2 --
               or spread * up: 4 + 1 -- and the sum): U_l = max(B_l + 2, U_{l+1} + 5) + 1 = U_{l+1} + 6.
               L levels: B_{L-1} = 51 + 6 L; U_0 = 51 + 6 L + 6 (L - 1).
  combine      up: 4, intensity * up: 1, rgb + that: 1.
  C(L) = 51 + 12 L.  Every term is non-negative after the bright pass's sanitising, so nothing else cancels; the one pixel of the
  test frame with negative channels is held to the same gate (|want| is then smaller than the terms)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from raytracing_folder_amd import capi
from tests import scenes
from tests.stage_support import F, ROOT, U, assert_driver_usage, build_driver, gi_params as _gi_params

DEFAULTS = dict(threshold=1.0, knee=0.5, intensity=0.25, spread=0.7, levels=6, exposure_ev=0.0)
CSRC = os.path.join(ROOT, "raytracing_folder_amd", "csrc")
TAIL_LIB = os.path.join(ROOT, "raytracing_folder_amd", "lib", "variants", "librt_bloom_tail.so")      # `make -C csrc bloom_tail`
TAIL_TEXELS = 5461              # RT_BLOOM_TAIL_TEXELS of that build (rt_bloom.hip): 64 KB of LDS at 12 bytes a texel


def gate_c(levels_used):
    return 51 + 12 * levels_used


# ---- the transcription --------------------------------------------------------------------------------------------
def ref_plan(w, h, levels):
    """step 3's level sizes [(w_l, h_l)]"""
    out = [((w + 1) // 2, (h + 1) // 2)]
    while len(out) < levels and out[-1] != (1, 1):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def _f(dt, a, b, c, d):
    return ((a + dt(3) * b) + (dt(3) * c + d)) * dt(0.125)


def _g(dt, n, f):
    return dt(0.75) * n + dt(0.25) * f


def ref_down(X, dt):
    h, w = X.shape[:2]
    ix = [np.clip(2 * np.arange((w + 1) // 2) + k - 1, 0, w - 1) for k in range(4)]
    iy = [np.clip(2 * np.arange((h + 1) // 2) + k - 1, 0, h - 1) for k in range(4)]
    R = _f(dt, X[:, ix[0]], X[:, ix[1]], X[:, ix[2]], X[:, ix[3]])
    return _f(dt, R[iy[0]], R[iy[1]], R[iy[2]], R[iy[3]])


def ref_up(X, fw, fh, dt):
    h, w = X.shape[:2]
    x, y = np.arange(fw), np.arange(fh)
    nx, ny = x >> 1, y >> 1
    fx = np.where(x & 1, np.minimum(nx + 1, w - 1), np.maximum(nx - 1, 0))
    fy = np.where(y & 1, np.minimum(ny + 1, h - 1), np.maximum(ny - 1, 0))
    near = _g(dt, X[ny][:, nx], X[ny][:, fx])
    far = _g(dt, X[fy][:, nx], X[fy][:, fx])
    return _g(dt, near, far)


def ref_bright(rgb, scale, threshold, knee, dt):
    with np.errstate(all="ignore"):
        rgb = np.asarray(rgb, F)
        c = np.where(np.isfinite(rgb) & (rgb >= 0), rgb, F(0)).astype(dt)
        Y = (dt(F(0.2126)) * c[..., 0] + dt(F(0.7152)) * c[..., 1]) + dt(F(0.0722)) * c[..., 2]
        Ys = dt(F(scale)) * Y
        t, k = dt(F(threshold)), dt(F(knee) * F(threshold))     # k is rounded to float once
        d = Ys - t
        x = np.minimum(np.maximum(d + k, dt(0)), dt(2) * k)
        s = (x * x) / (dt(4) * k + dt(F(1e-5)))
        wgt = np.maximum(s, d) / np.maximum(Ys, dt(F(1e-5)))
        wgt = np.where((t == 0) | ~np.isfinite(Ys), dt(1), wgt).astype(dt)
        return c * wgt[..., None]


def ref_bloom(rgb, scale=1.0, dtype=np.float64, **kw):
    """(out, up(U_0)) of the definition"""
    p = dict(DEFAULTS, **kw)
    p.pop("exposure_ev")                                        # the caller turns it into `scale`
    dt = dtype
    rgb = np.asarray(rgb, F)
    h, w = rgb.shape[:2]
    with np.errstate(all="ignore"):
        B = [ref_down(ref_bright(rgb, scale, p["threshold"], p["knee"], dt), dt)]
        for _ in ref_plan(w, h, p["levels"])[1:]:
            B.append(ref_down(B[-1], dt))
        a, spread = dt(F(1) - F(p["spread"])), dt(F(p["spread"]))       # a is rounded to float once
        Uc = B[-1]
        for Bl in B[-2::-1]:
            Uc = a * Bl + spread * ref_up(Uc, Bl.shape[1], Bl.shape[0], dt)
        bloom = ref_up(Uc, w, h, dt)
        return rgb.astype(dt) + dt(F(p["intensity"])) * bloom, bloom


def worst_over_gate(got, want, levels_used):
    """worst error / gate over the finite entries; where the transcription is not finite the other side is the same kind"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert (np.isnan(got) == np.isnan(want)).all()
    assert (got[~fin & ~np.isnan(want)] == want[~fin & ~np.isnan(want)]).all()
    gate = gate_c(levels_used) * U * np.abs(want[fin]) + 1e-7
    return float((np.abs(got[fin] - want[fin]) / gate).max()) if fin.any() else 0.0


# ---- the frames -------------------------------------------------------------------------------------------------------
def _pixel_for(Y):
    """a pixel with one channel set whose luminance is Y exactly: fl(coefficient * v) == Y, the other terms and the sums are
    exact zeros.  Which channel has such a v depends on the binades of Y and v: the first that has one is taken"""
    for ch, coef in ((1, F(0.7152)), (0, F(0.2126)), (2, F(0.0722))):
        v = F(float(Y) / float(coef))
        for _ in range(16):
            got = coef * v
            if got == Y:
                px = [F(0), F(0), F(0)]
                px[ch] = v
                return tuple(px)
            v = np.nextafter(v, F(np.inf) if got < Y else F(-np.inf))
    raise AssertionError(Y)


SPECIAL = 8         # the pixels hdr_frame plants, from the middle of the middle row on


def hdr_frame(w, h, seed=1, lo=-8.0, hi=8.0, special=True):
    """float32 (h, w, 3): luminances log-uniform over 2^lo .. 2^hi and -- where the frame has room -- a zero pixel, one with a
    negative channel, a NaN and a +inf pixel, and pixels whose Ys (scale 1) is exactly the threshold 1 and exactly the knee's
    ends 0.5 and 1.5"""
    rng = np.random.default_rng(seed)
    Y = 2.0 ** rng.uniform(lo, hi, (h, w))
    lin = (Y[..., None] * rng.uniform(0.5, 1.5, (h, w, 3))).astype(F)
    if special and w * h >= 64:
        flat = lin.reshape(-1, 3)
        at = w * (h // 2) + w // 2
        vals = [(0, 0, 0), (0.75, -0.25, 3), (np.nan, np.nan, np.nan), (np.inf, 1, 1), (0, 0, 0)] + [_pixel_for(F(y)) for y in (1.0, 0.5, 1.5)]
        assert len(vals) == SPECIAL
        for k, v in enumerate(vals):
            flat[at + k] = v
    return lin


def ref_tail_level(w, h, levels=6):
    """the level k_bloom_tail starts at in the build that has it: the first that fits TAIL_TEXELS together with every level below
    it and leaves the kernel at least two levels; -1 when there is none.  The shipped build has no tail kernel."""
    texels = [a * b for a, b in ref_plan(w, h, levels)]
    for t in range(len(texels) - 1):
        if sum(texels[t:]) <= TAIL_TEXELS:
            return t
    return -1


# 128 x 128: level 0 is 64 x 64 and 4096 + 1024 + 256 + 64 + 16 + 4 = 5460 texels fit, so the tail kernel starts exactly at level 0;
# 130 x 130 is one level-0 texel larger each way (65 x 65: 5718 texels), where it starts at level 1
TAIL_SIZES = [(128, 128), (130, 130)]
SIZES = [(1, 1), (1, 7), (2, 2), (3, 2), (5, 40), (37, 23), (64, 64), (130, 66)] + TAIL_SIZES


_REF = {}


def reference(w, h, levels, dtype=np.float64):
    """the transcription of hdr_frame(w, h) at the default parameters and `levels`, computed once and shared"""
    key = (w, h, levels, dtype)
    if key not in _REF:
        _REF[key] = ref_bloom(hdr_frame(w, h), 1.0, dtype, levels=levels)
    return _REF[key]


# ---- without a GPU -------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("rt_bloom_create", "rt_bloom_destroy", "rt_bloom_default_params", "rt_bloom_plan", "rt_bloom_device", "rt_bloom_host")


def test_new_symbols_struct_layout_and_defaults():
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert L.rt_abi_version() == 4
    assert [f[0] for f in capi.BloomParams._fields_] == ["struct_size", "threshold", "knee", "intensity", "spread", "levels", "exposure_ev"]
    assert [f[0] for f in capi.BloomPlanes._fields_] == ["struct_size", "rgb_linear", "out", "out_bloom"]
    assert C.sizeof(capi.BloomParams) == 28 and C.sizeof(capi.BloomPlanes) == 32
    p = capi.BloomParams()
    L.rt_bloom_default_params(C.byref(p))
    assert p.struct_size == 28
    for k, v in DEFAULTS.items():
        assert getattr(p, k) == (v if k == "levels" else F(v)), k
    L.rt_bloom_default_params(None)                             # ignored
    L.rt_bloom_destroy(None)                                    # ignored
    with pytest.raises(TypeError):
        capi.bloom_params(gamma=2.2)
    # the existing structs did not grow
    assert C.sizeof(capi.ToneMapParams) == 52 and C.sizeof(capi.ToneMapPlanes) == 40 and C.sizeof(capi.Outputs) == 72


def test_plan_equals_the_transcription():
    for w, h in SIZES + [(1920, 1080), (1, 4096), (7, 1)]:
        for levels in (1, 2, 6, 31):
            used, tail = capi.bloom_plan(w, h, levels)
            plan = ref_plan(w, h, levels)
            assert used == len(plan), (w, h, levels)
            assert tail == -1                                   # the shipped build runs every level as a launch of its own
            assert ref_tail_level(w, h, levels) < used - 1
            if len(plan) < levels:
                assert plan[-1] == (1, 1) and (len(plan) == 1 or plan[-2] != (1, 1))
    assert capi.bloom_plan(1, 1) == (1, -1) and capi.bloom_plan(3, 2)[0] == 2 and capi.bloom_plan(130, 66)[0] == 6
    L = capi.lib()
    assert L.rt_bloom_plan(0, 4, 6, None, None) == -1 and L.rt_bloom_plan(4, 4, 0, None, None) == -1
    # the sizes the tail build is tested at: exactly at level 0, and just not; 1080p from level 4
    assert [ref_tail_level(*s) for s in TAIL_SIZES] == [0, 1] and ref_tail_level(1920, 1080) == 4 and ref_tail_level(1, 1) == -1


def _arg_cases():
    buf = np.zeros(8 * 8 * 3 * 3, np.float32)
    ptr = buf.ctypes.data
    full = lambda **kw: capi.BloomPlanes(**{**dict(rgb_linear=ptr, out=ptr, out_bloom=ptr + 8 * 8 * 12), **kw})
    nan, inf = float("nan"), float("inf")
    cases = []
    for bad in (0, 27, 32):
        p = capi.bloom_params()
        p.struct_size = bad
        cases.append((b"struct_size", p, full()))
    pl = full()
    pl.struct_size += 8
    cases.append((b"struct_size", capi.bloom_params(), pl))
    for name in ("threshold", "knee", "intensity", "spread"):
        for bad in (-0.5, nan, inf):
            cases.append((b"finite and not negative", capi.bloom_params(**{name: bad}), full()))
    cases.append((b"at most 1", capi.bloom_params(spread=1.5), full()))
    cases.append((b"at most 1", capi.bloom_params(knee=1.25), full()))
    for bad in (0, -2):
        cases.append((b"levels is", capi.bloom_params(levels=bad), full()))
    for bad in (nan, inf):
        cases.append((b"exposure_ev", capi.bloom_params(exposure_ev=bad), full()))
    cases.append((b"rgb_linear is required", capi.bloom_params(), full(rgb_linear=None)))
    cases.append((b"one of out and out_bloom", capi.bloom_params(), full(out=None, out_bloom=None)))
    return buf, cases, full


def test_argument_checks_come_before_any_gpu_call():
    """every check that does not need the object is reached with a NULL one, so it is reached without a device; the two that do
    (an exposure state on another device, overlapping planes) are in test_argument_checks_with_an_object"""
    L = capi.lib()
    buf, cases, full = _arg_cases()
    for what, p, pl in cases:
        for st in (L.rt_bloom_host(None, None, C.byref(p), C.byref(pl)), L.rt_bloom_device(None, None, None, C.byref(p), C.byref(pl), 1)):
            assert st == -1 and what in L.rt_last_error(), (what, L.rt_last_error())
    p, pl = capi.bloom_params(), full()
    for args in ((None, C.byref(pl)), (C.byref(p), None)):
        assert L.rt_bloom_host(None, None, *args) == -1 and L.rt_bloom_device(None, None, None, *args, 1) == -1
    assert L.rt_bloom_host(None, None, C.byref(p), C.byref(pl)) == -1 and b"rt_bloom is NULL" in L.rt_last_error()
    h = C.c_void_p()
    for w_, h_ in ((0, 8), (8, 0), (-3, 8)):
        assert L.rt_bloom_create(0, w_, h_, C.byref(h)) == -1 and b"bad image size" in L.rt_last_error() and not h
    assert L.rt_bloom_create(0, 8, 8, None) == -1
    # more than 2^30 pixels: RT_ERR_LIMIT, after the argument checks and before the device is looked for
    assert L.rt_bloom_create(0, 1 << 16, (1 << 14) + 1, C.byref(h)) == -6 and b"2^30" in L.rt_last_error() and not h
    if capi.device_count() == 0:                                # ... and RT_ERR_NO_DEVICE comes after all of them
        assert L.rt_bloom_create(0, 8, 8, C.byref(h)) == -3 and not h
        with pytest.raises(capi.RtError) as err:
            capi.Bloom(0, 8, 8)
        assert err.value.status == -3


def test_shim_driver_builds_against_the_header(tmp_path):
    assert_driver_usage(build_driver(tmp_path, "shim_bloom_driver"))


def test_frame_holds_what_the_tests_rely_on():
    lin = hdr_frame(37, 23)
    c = np.where(np.isfinite(lin) & (lin >= 0), lin, F(0))
    Y = (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]
    for y in (1.0, 0.5, 1.5):
        assert (Y == F(y)).sum() == 1
    assert np.isnan(lin).any(axis=2).sum() == 1 and np.isposinf(lin).any(axis=2).sum() == 1 and (lin < 0).any(axis=2).sum() == 1
    assert (lin == 0).all(axis=2).sum() == 2
    fin = Y[Y > 0]
    assert fin.min() < 2.0 ** -7 and fin.max() > 2.0 ** 7
    P = ref_bright(lin, 1.0, 1.0, 0.5, np.float64)
    wgt = lambda y: P[Y == F(y)][0].sum() / float(sum(_pixel_for(F(y))))
    # (in double the product that rounds to Y in float is off by up to 2^-24 Y: the transcription's pixel is NEAR the knee's end)
    assert wgt(0.5) < 1e-15 and abs(wgt(1.5) - 1 / 3) < 1e-7 and abs(wgt(1.0) - 0.125 / (1 + 0.5e-5)) < 1e-7
    assert not P[np.isnan(lin).any(axis=2)].any() and np.isfinite(P).all()                     # NaN and inf channels count as 0 ...
    assert (P[np.isposinf(lin).any(axis=2)][0] > 0).tolist() == [False, True, True]             # ... and the pixel's other channels stay
    assert ((Y > 0.5) & (Y < 1.5)).sum() > 20                   # pixels inside the knee


@pytest.mark.parametrize("size", SIZES + [(199, 201)], ids=lambda s: f"{s[0]}x{s[1]}")          # and one larger, odd both ways
def test_reference_partition_of_unity_and_pass_through(size):
    """a constant frame with threshold 0 is c (1 + intensity) everywhere, edges and odd sizes included; a frame wholly below
    threshold * (1 - knee) comes back unchanged"""
    w, h = size
    for levels in (1, 2, 6):
        for c, intensity, spread in ((0.5, 0.25, 0.7), (3.0, 1.0, 0.0), (1e-7, 0.5, 1.0)):
            frame = np.full((h, w, 3), c, F) * np.array([1.0, 0.5, 0.25], F)
            out, bloom = ref_bloom(frame, 1.0, threshold=0.0, levels=levels, intensity=intensity, spread=spread)
            want = frame.astype(np.float64) * (1 + float(F(intensity)))
            assert np.abs(out - want).max() <= 64 * 2.0 ** -53 * want.max(), (levels, c)
            assert np.abs(bloom - frame).max() <= 64 * 2.0 ** -53 * frame.max()
        dark = hdr_frame(w, h, lo=-8.0, hi=-2.0, special=False)        # channels below 1.5 * 2^-2: Ys < 0.5 = t (1 - knee)
        out, bloom = ref_bloom(dark, 1.0, levels=levels)
        assert (out == dark).all() and not bloom.any()
        out, bloom = ref_bloom(dark * F(64), 1.0 / 64, levels=levels)  # the threshold is relative to the scale
        assert (out == dark * F(64)).all() and not bloom.any()


def test_reference_symmetry_nan_isolation_and_levels():
    frame = np.zeros((64, 64, 3), F)
    frame[31:33, 31:33] = (40.0, 20.0, 10.0)
    out, bloom = ref_bloom(frame)
    assert (bloom == bloom[:, ::-1]).all() and (bloom == bloom[::-1]).all() and bloom[0, 0, 0] > 0 and bloom[32, 32, 0] > bloom[20, 20, 0]
    lin = hdr_frame(37, 23)
    nan_at = np.isnan(lin).any(axis=2)
    zeroed = lin.copy()
    zeroed[nan_at] = 0
    a, b = ref_bloom(lin)[0], ref_bloom(zeroed)[0]
    assert np.isnan(a[nan_at][0, 0]) and (a[~nan_at] == b[~nan_at]).all()
    small = hdr_frame(3, 2)
    assert (ref_bloom(small, levels=6)[1] == ref_bloom(small, levels=2)[1]).all()  # 3 x 2 has two levels (2 x 1, 1 x 1): 6 is clipped
    assert (ref_bloom(lin, levels=2)[1] != ref_bloom(lin, levels=1)[1]).any()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_counted_gate_holds_for_a_float32_evaluation(size):
    w, h = size
    worst = 0.0
    for levels in (1, 2, 6):
        used = len(ref_plan(w, h, levels))
        want, got = reference(w, h, levels), reference(w, h, levels, np.float32)
        # no exp2 in this evaluation: 2u less on Ys, which the bright pass hands on three times (the subtraction's factor)
        worst = max(worst, max(worst_over_gate(g, wt, used) for g, wt in zip(got, want)) * gate_c(used) / (gate_c(used) - 6))
    print(f"bloom float32 evaluation {w}x{h}: worst error / gate {worst:.3f}")
    assert worst <= 1.0


def test_counted_gate_holds_across_the_knee():
    """the bright pass alone, pixel by pixel, swept through the knee and above it, for pixels of the frames' kind (channels within
    0.5 .. 1.5 of one value) at three scales"""
    rng = np.random.default_rng(7)
    for scale in (1.0, 0.3712, 2.0 ** 3):
        Ys = rng.uniform(0.4, 2.5, (200000, 1)) / scale
        px = (Ys * rng.uniform(0.5, 1.5, (200000, 3))).astype(F)
        want, got = ref_bright(px, scale, 1.0, 0.5, np.float64), ref_bright(px, scale, 1.0, 0.5, np.float32)
        gate = 51 * U * np.abs(want) + 1e-7
        assert (np.abs(got - want) <= gate).all(), float((np.abs(got - want) / gate).max())


# ---- on the GPU ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_against_the_float64_transcription(size):
    w, h = size
    lin = hdr_frame(w, h)
    worst = 0.0
    with capi.Bloom(0, w, h) as bl:
        for levels in (1, 2, 6):
            used = capi.bloom_plan(w, h, levels)[0]
            out, bloom = bl.apply(lin, return_bloom=True, levels=levels)
            want_out, want_bloom = reference(w, h, levels)
            worst = max(worst, worst_over_gate(out, want_out, used), worst_over_gate(bloom, want_bloom, used))
    print(f"bloom {w}x{h}: worst error / gate {worst:.3f} (gate (51 + 12 L) * 2^-24 * |want| + 1e-7)")
    assert worst <= 1.0


@pytest.mark.gpu
def test_exact_properties_on_the_device():
    import torch
    lin = hdr_frame(37, 23)
    clean = hdr_frame(37, 23, special=False)
    with capi.Bloom(0, 37, 23) as bl, capi.Bloom(0, 64, 64) as bl64:
        assert bl.apply(clean, intensity=0.0).tobytes() == clean.tobytes()
        dark = hdr_frame(37, 23, lo=-8.0, hi=-2.0, special=False)
        out, bloom = bl.apply(dark, return_bloom=True)
        assert out.tobytes() == dark.tobytes() and not bloom.any()
        # a constant frame at threshold 0: the partition of unity, edges included
        frame = np.full((64, 64, 3), 0.5, F) * np.array([1.0, 0.5, 0.25], F)
        out = bl64.apply(frame, threshold=0.0, intensity=0.5)
        want = frame.astype(np.float64) * 1.5
        assert (np.abs(out - want) <= gate_c(6) * U * want + 1e-7).all()
        # a 2 x 2 bright block in the centre of a black frame: the response equals its own flips
        frame = np.zeros((64, 64, 3), F)
        frame[31:33, 31:33] = (40.0, 20.0, 10.0)
        _, bloom = bl64.apply(frame, return_bloom=True)
        g = gate_c(6) * U * np.abs(bloom.astype(np.float64)) + 1e-7
        assert (np.abs(bloom - bloom[:, ::-1]) <= g).all() and (np.abs(bloom - bloom[::-1]) <= g).all() and bloom[0, 0, 0] > 0
        # twice the same call, and in place against out of place on device planes
        first, again = bl.apply(lin, return_bloom=True), bl.apply(lin, return_bloom=True)
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(device=dev)
        src = torch.from_numpy(lin).to(dev)
        inplace, outp, only = src.clone(), torch.zeros_like(src), torch.zeros_like(src)
        torch.cuda.synchronize()
        bl.apply_device(side.cuda_stream, linear_ptr=src.data_ptr(), out_ptr=outp.data_ptr(), bloom_ptr=only.data_ptr())
        bl.apply_device(side.cuda_stream, linear_ptr=inplace.data_ptr(), out_ptr=inplace.data_ptr(), sync=True)
        assert outp.cpu().numpy().tobytes() == first[0].tobytes() == inplace.cpu().numpy().tobytes()
        assert only.cpu().numpy().tobytes() == first[1].tobytes() and src.cpu().numpy().tobytes() == lin.tobytes()
        only.zero_()
        bl.apply_device(side.cuda_stream, linear_ptr=src.data_ptr(), out_ptr=None, bloom_ptr=only.data_ptr(), sync=True)
        assert only.cpu().numpy().tobytes() == first[1].tobytes()
        # the NaN pixel stays NaN and changes no other pixel
        nan_at = np.isnan(lin).any(axis=2)
        zeroed = lin.copy()
        zeroed[nan_at] = 0
        b = bl.apply(zeroed)
        assert np.isnan(first[0][nan_at][0, 0]) and first[0][~nan_at].tobytes() == b[~nan_at].tobytes()


@pytest.mark.gpu
def test_argument_checks_with_an_object():
    import torch
    L = capi.lib()
    t = torch.zeros((8 * 8 * 3 * 3,), dtype=torch.float32, device="cuda:0")
    ptr = t.data_ptr()
    n = 8 * 8 * 12
    p = capi.bloom_params()
    with capi.Bloom(0, 8, 8) as bl, capi.Exposure(0) as exp:
        _, cases, _ = _arg_cases()
        for what, bad, pl in cases:                             # the same refusals with an object
            assert L.rt_bloom_host(bl._h, None, C.byref(bad), C.byref(pl)) == -1 and what in L.rt_last_error(), what
        for pl in (capi.BloomPlanes(rgb_linear=ptr, out=ptr + 12), capi.BloomPlanes(rgb_linear=ptr, out=ptr, out_bloom=ptr + n - 4),
                   capi.BloomPlanes(rgb_linear=ptr, out=ptr + n, out_bloom=ptr + n), capi.BloomPlanes(rgb_linear=ptr, out_bloom=ptr)):
            assert L.rt_bloom_device(bl._h, None, None, C.byref(p), C.byref(pl), 1) == -1 and b"overlap" in L.rt_last_error()
        ok = capi.BloomPlanes(rgb_linear=ptr, out=ptr, out_bloom=ptr + n)
        assert L.rt_bloom_device(bl._h, exp._h, None, C.byref(p), C.byref(ok), 1) == 0
        if capi.device_count() > 1:
            with capi.Exposure(1) as other:
                assert L.rt_bloom_device(bl._h, other._h, None, C.byref(p), C.byref(ok), 1) == -1 and b"on device 1" in L.rt_last_error()


@pytest.mark.gpu
def test_threshold_is_relative_to_the_exposure_state():
    lin = hdr_frame(37, 23)
    used = capi.bloom_plan(37, 23)[0]
    with capi.Bloom(0, 37, 23) as bl, capi.Exposure(0) as exp:
        for ev in (0.0, -1.5):
            want = ref_bloom(lin, F(2.0 ** float(F(ev))))       # a fresh state holds no metered frame: 2^exposure_ev, like None
            for state in (None, exp):
                got = bl.apply(lin, exposure=state, return_bloom=True, exposure_ev=ev)
                assert max(worst_over_gate(g, wt, used) for g, wt in zip(got, want)) <= 1.0, (ev, state)
        assert exp.metered_pixels == 0 and not exp.histogram().any()
        exp.tonemap(lin * F(8), key=0.36)
        hist, E, n = exp.histogram(), exp.log2_exposure, exp.metered_pixels
        assert abs(E) > 0.5
        got = bl.apply(lin, exposure=exp, return_bloom=True, exposure_ev=3.0)          # exposure_ev is not used now
        want = ref_bloom(lin, F(2.0 ** float(F(E))))
        worst = max(worst_over_gate(g, wt, used) for g, wt in zip(got, want))
        print(f"bloom with a metered state: E {E:.4f}, worst error / gate {worst:.3f}")
        assert worst <= 1.0
        assert got[1].tobytes() != bl.apply(lin, return_bloom=True)[1].tobytes()
        assert (exp.histogram() == hist).all() and exp.log2_exposure == E and exp.metered_pixels == n      # only read


_CHILD = """
import sys
import numpy as np
import torch
from raytracing_folder_amd import capi
from tests import test_bloom as T
out = {}
for w, h in T.SIZES:
    for levels in (1, 2, 6):
        assert capi.bloom_plan(w, h, levels) == (len(T.ref_plan(w, h, levels)), T.ref_tail_level(w, h, levels)), (w, h, levels)
    with capi.Bloom(0, w, h) as bl:
        out[f"f{w}x{h}_out"], out[f"f{w}x{h}_bloom"] = bl.apply(T.hdr_frame(w, h), return_bloom=True)
np.savez(sys.argv[1], **out)
"""


@pytest.mark.gpu
def test_the_build_with_the_tail_kernel_agrees(tmp_path):
    """`make bloom_tail`: the library whose small levels k_bloom_tail runs inside LDS, in a process of its own, at every size --
    the two tail-boundary sizes among them: inside the gate against the transcription and against the shipped build"""
    if not os.path.exists(TAIL_LIB):
        subprocess.run(["make", "-s", "-C", CSRC, "bloom_tail"], check=True, capture_output=True, timeout=600)
    dst = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, dst], env=dict(os.environ, RT_MI355X_LIB=TAIL_LIB, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, (r.stdout, r.stderr)
    other = np.load(dst)
    assert sorted({ref_tail_level(w, h) for w, h in SIZES}) == [-1, 0, 1]           # no tail, from level 0, from a later level
    worst = 0.0
    for w, h in SIZES:
        with capi.Bloom(0, w, h) as bl:
            mine = bl.apply(hdr_frame(w, h), return_bloom=True)
        want = reference(w, h, 6)
        used = capi.bloom_plan(w, h)[0]
        for k, name in enumerate(("out", "bloom")):
            got = other[f"f{w}x{h}_{name}"]
            worst = max(worst, worst_over_gate(got, want[k], used))
            g = gate_c(used) * U * np.abs(want[k]) + 1e-7
            fin = np.isfinite(want[k])
            assert (np.abs(got[fin].astype(np.float64) - mine[k][fin]) <= g[fin]).all(), (w, h, name)
    print(f"bloom, the build with k_bloom_tail: worst error / gate {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.gpu
def test_render_denoised_and_render_temporal_with_a_bloom():
    """cornell_gi.xml, live GI, 96 x 72, 4 spp, reproducible mode"""
    s, cam = scenes.load_cornell_gi(96, 72)
    s.set_render_flags(capi.RENDER_REPRODUCIBLE)
    kw = dict(threshold=0.1, intensity=0.5)                     # the frame is dim: its denoised plane peaks near 0.2
    with capi.Exposure(0) as before:                            # the same call before any Bloom exists
        plain = s.render_denoised(cam, _gi_params(1), exposure=before, tonemap_kw=dict(operator="clamp"))
    with capi.Bloom(0, 96, 72) as bl, capi.Exposure(0) as exp, capi.Exposure(0) as twin:
        with capi.Exposure(0) as again:
            same = s.render_denoised(cam, _gi_params(1), exposure=again, tonemap_kw=dict(operator="clamp"))
        assert set(same) == set(plain)
        for k, v in plain.items():
            if isinstance(v, np.ndarray):
                assert same[k].tobytes() == v.tobytes(), k
        for frame, seed in enumerate((1, 2)):                   # the second frame is bloomed relative to the first one's exposure
            out = s.render_denoised(cam, _gi_params(seed), exposure=exp, bloom=bl, bloom_kw=kw, tonemap_kw=dict(operator="clamp"))
            assert set(out) == set(plain) | {"bloomed"}
            want = bl.apply(out["denoised"], exposure=twin, **kw)       # twin holds what exp held when the frame was bloomed
            assert out["bloomed"].tobytes() == want.tobytes() and out["bloomed"].tobytes() != out["denoised"].tobytes()
            assert out["display_rgb"].tobytes() == twin.tonemap(out["bloomed"], out["object_id"], operator="clamp", gamma=_gi_params(1).gamma).tobytes()
            assert twin.log2_exposure == exp.log2_exposure
            if frame == 0:
                for k, v in plain.items():
                    if isinstance(v, np.ndarray) and k != "display_rgb":
                        assert out[k].tobytes() == v.tobytes(), k
                assert out["display_rgb"].tobytes() != plain["display_rgb"].tobytes()
        with capi.History(0, 96, 72) as hst, capi.History(0, 96, 72) as hst_plain:
            exp.reset()
            out = s.render_temporal(hst, cam, _gi_params(3), denoise=False, exposure=exp, bloom=bl, bloom_kw=kw)
            ref = s.render_temporal(hst_plain, cam, _gi_params(3), denoise=False)
            assert set(out) == set(ref) | {"bloomed", "display_rgb"}
            for k, v in ref.items():
                if isinstance(v, np.ndarray):
                    assert out[k].tobytes() == v.tobytes(), k
            assert out["bloomed"].tobytes() == bl.apply(out["accumulated"], **kw).tobytes()


@pytest.mark.gpu
def test_cpp_shim_bloom_equals_the_capi_one(tmp_path):
    exe = build_driver(tmp_path, "shim_bloom_driver")
    prefix = str(tmp_path / "f")
    r = subprocess.run([exe, scenes.CORNELL, prefix, "64", "48"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    s, cam = scenes.load_cornell(64, 48)
    s.set_render_flags(capi.RENDER_REPRODUCIBLE)
    p = capi.default_params(shade_model=capi.SHADE_P13, bounce=6, photon_count=0, min_sample=4, max_sample=8, threshold=1e-3, seed=11)
    with capi.Exposure(0) as exp, capi.Bloom(0, 64, 48) as bl:
        for frame in (1, 2):
            p.seed = 10 + frame
            one = s.render_outputs(cam, p, planes=("linear", "object_id"))
            bloomed = bl.apply(one["linear"], exposure=exp, threshold=0.5, intensity=0.5)
            rgb = exp.tonemap(bloomed, one["object_id"])
            assert capi.image_read_pfm(f"{prefix}_bloom{frame}.pfm").tobytes() == bloomed.tobytes(), frame
            assert open(f"{prefix}_rgb{frame}.bin", "rb").read() == rgb.tobytes(), frame
            assert bloomed.tobytes() != one["linear"].tobytes()
        assert np.float32(float(r.stdout.split()[-1])) == np.float32(exp.log2_exposure)
