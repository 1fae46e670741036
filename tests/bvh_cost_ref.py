"""The yardstick of the mesh tree quality tests (include/rt_mi355x.h, "mesh tree quality"): the SAH cost of DEVBVHNODE records by
numpy.  The per-term half areas and weights are float32 in the stated operation order; the SUM is math.fsum over the terms in
float64 -- exactly rounded, which is NOT the fixed order of additions the library's two implementations follow, so this is
independent of both.  The tolerance against it is 1e-9 relative: fewer than 2^20 double additions of non-negative terms stay within
2^20 * 2^-53 = 1.2e-10 relative of the exact sum, and the last division adds one rounding.

refit() emulates k_bvh_refit_level on the host (every used child's box becomes the float min / max of the vertices beneath it; refs
stay), so that the CPU tests can check the deformations the GPU tests rely on."""
import math

import numpy as np

from raytracing_folder_amd import capi

F = np.float32
LEAF = capi.DEVBVH_LEAF
RTOL = 1e-9


def _half_area(lo, hi):
    d = (hi - lo).astype(F)
    return ((d[..., 0] * d[..., 1]).astype(F) + (d[..., 1] * d[..., 2]).astype(F)).astype(F) + (d[..., 2] * d[..., 0]).astype(F)


def terms(nodes):
    """[n_nodes, 4] float32: term(n, c), 0 for unused children"""
    lo, hi, c = np.moveaxis(nodes["lo"], 1, 2), np.moveaxis(nodes["hi"], 1, 2), nodes["c"]          # [n, child, axis]
    with np.errstate(all="ignore"):
        h = _half_area(lo, hi).astype(F)
        w = np.where(c & LEAF, ((c >> 28) & 7) + 1, 1).astype(F)
        return np.where(np.isnan(nodes["lo"][:, 0, :]), F(0), (h * w).astype(F)).astype(F)


def root_half_area(nodes, root_ref):
    r = nodes[int(root_ref)]
    used = ~np.isnan(r["lo"][0])
    return _half_area(r["lo"][:, used].min(1)[None], r["hi"][:, used].max(1)[None])[0]


def sah_cost(nodes, root_ref):
    """the cost by the definition with an exactly rounded sum; None where the definition says degenerate"""
    root_ref = int(root_ref)
    if root_ref & LEAF:
        return 1.0 + (((root_ref >> 28) & 7) + 1)
    S = math.fsum(terms(nodes).astype(np.float64).ravel().tolist())
    HR = float(root_half_area(nodes, root_ref))
    if HR == 0.0 or not math.isfinite(HR) or not math.isfinite(S):
        return None
    return 1.0 + S / HR


def refit(nodes, slot_face, v, f):
    """a copy of `nodes` refitted to the vertices v: the box of every used child is the min / max of the vertices of the faces
    beneath it"""
    out = nodes.copy()
    memo = {}

    def beneath(ref):
        ref = int(ref)
        if ref & LEAF:
            first = ref & 0x0FFFFFFF
            return slot_face[first:first + ((ref >> 28) & 7) + 1]
        if ref not in memo:
            used = ~np.isnan(nodes["lo"][ref][0])
            memo[ref] = np.concatenate([beneath(nodes["c"][ref][k]) for k in np.nonzero(used)[0]])
        return memo[ref]
    for i in range(len(nodes)):
        for ch in range(4):
            if np.isnan(nodes["lo"][i][0][ch]):
                continue
            p = v[f[beneath(nodes["c"][i][ch])]].reshape(-1, 3)
            out["lo"][i][:, ch], out["hi"][i][:, ch] = p.min(0), p.max(0)
    return out
