"""The float64 yardstick of "motion vectors for deforming meshes" (include/rt_mi355x.h): steps a'-e' transcribed from the header,
with a brute-force ray test over ALL triangles of the mesh in place of the tree, on top of test_motion.ref_motion for the rigid
pixels.  Shared by tests/test_motion_mesh.py's CPU and GPU tests; nothing here touches the library."""
import math

import numpy as np

from tests.test_motion import from_object, ref_motion, to_object
from tests.stage_support import BIG, F
from tests.test_temporal import cam_setup

BIAS_FIN = 1e-3                         # tri_hit_fin accepts t > 0.001
EDGE_PX = 0.01                          # a pixel is left out when a ray 0.01 px beside its centre decides otherwise (see near_decision)
GATE_MARGIN = 1e-4                      # ... or when | |t - z| / z - depth_tol | is below this


def rays_at(cs, dx=0.0, dy=0.0):
    """pixel_rays of test_temporal through (x + 0.5 + dx, y + 0.5 + dy): unit directions (H, W, 3), float64"""
    Y, X = np.mgrid[0:cs["H"], 0:cs["W"]]
    s = np.stack([cs["b"][0] + (X + 0.5 + dx) * cs["u"], cs["b"][1] + (Y + 0.5 + dy) * cs["v"], np.full(X.shape, cs["b"][2])], -1)
    d = s @ cs["M"].T
    return d / np.sqrt((d * d).sum(-1))[..., None]


def closest(v, f, o, d):
    """brute force: the closest hit of every ray (o, d) [n, 3] with every triangle, two-sided, t > BIAS_FIN; returns (t [n] (inf:
    miss), face [n], bc [n, 3] the weights of the face's three vertices)"""
    v = np.asarray(v, np.float64)
    A, B, C = (v[f[:, k]] for k in range(3))
    e1, e2 = B - A, C - A
    n, chunk = len(o), max(16, 200000 // len(f))
    best_t, best_f, best_bc = np.full(n, np.inf), np.zeros(n, np.int64), np.zeros((n, 3))
    for lo in range(0, n, chunk):
        oo, dd = o[lo:lo + chunk, None, :], d[lo:lo + chunk, None, :]
        with np.errstate(all="ignore"):
            pv = np.cross(dd, e2[None])
            det = (e1[None] * pv).sum(-1)
            tv = oo - A[None]
            u = (tv * pv).sum(-1) / det
            qv = np.cross(tv, e1[None])
            w = (dd * qv).sum(-1) / det
            t = (e2[None] * qv).sum(-1) / det
            ok = (det != 0) & (u >= 0) & (w >= 0) & (u + w <= 1) & (t > BIAS_FIN)
        t = np.where(ok, t, np.inf)
        k = t.argmin(1)
        r = np.arange(len(k))
        best_t[lo:lo + chunk], best_f[lo:lo + chunk] = t[r, k], k
        best_bc[lo:lo + chunk] = np.stack([1 - u[r, k] - w[r, k], u[r, k], w[r, k]], -1)
    return best_t, best_f, best_bc


def object_rays(cs, nodes, i, dx=0.0, dy=0.0):
    """a'.: the rays of all pixels in node i's object coordinates, (o [n, 3], d [n, 3]); d is NOT renormalised"""
    d = rays_at(cs, dx, dy).reshape(-1, 3)
    o = np.broadcast_to(cs["pos"], d.shape)
    oo = to_object(nodes, i, o)
    return oo, to_object(nodes, i, o + d) - oo


def synthetic_planes(cam, nodes, mesh_node, v, f, jitter=(0.0, 0.0)):
    """the z and object_id planes a render of the mesh alone would give, from the ray `jitter` pixels beside each pixel's centre (a
    jittered sample): z = float32(t) and id = mesh_node where it hits, (BIG, -1) elsewhere"""
    cs = cam_setup(cam)
    o, d = object_rays(cs, nodes, mesh_node, *jitter)
    t, _, _ = closest(v, f, o, d)
    hit = np.isfinite(t).reshape(cs["H"], cs["W"])
    z = np.where(hit, t.reshape(hit.shape), BIG).astype(F)
    return z, np.where(hit, mesh_node, -1).astype(np.int32)


def ref_motion_mesh(cam, prev_cam, nodes, prev_nodes, mesh_nodes, z, ids, depth_tol=0.05):
    """float64 transcription of the section.  mesh_nodes: {node index: (v, v_prev, f)} of the nodes whose mesh holds previous
    positions.  Returns (plane (H, W, 3), found (H, W), near (H, W): pixels whose hit or gate decision lies within the margins)"""
    cs, old = cam_setup(cam), cam_setup(prev_cam)
    H, W = cs["H"], cs["W"]
    out, found, _ = ref_motion(cam, prev_cam, nodes, prev_nodes, z, ids)
    out, found = out.copy(), found.copy()
    near = np.zeros((H, W), bool)
    with np.errstate(all="ignore"):
        ok = (ids >= 0) & (ids < len(nodes)) & np.isfinite(z) & (z < BIG)
    Y, X = np.mgrid[0:H, 0:W]
    for i, (v, v_prev, f) in mesh_nodes.items():
        m = (ok & (ids == i)).reshape(-1)
        if not m.any():
            continue
        o, d = object_rays(cs, nodes, i)
        t, face, bc = closest(v, f, o[m], d[m])
        zz = z.reshape(-1)[m].astype(np.float64)
        hit = np.isfinite(t)
        with np.errstate(all="ignore"):
            rel = np.abs(t - zz) / zz
        passed = hit & ~(rel > depth_tol)
        vp = np.asarray(v_prev, np.float64)
        Xo = (bc[:, 0:1] * vp[f[face, 0]] + bc[:, 1:2] * vp[f[face, 1]]) + bc[:, 2:3] * vp[f[face, 2]]
        Pp = from_object(prev_nodes if prev_nodes is not None else nodes, i, Xo)
        e = Pp - old["pos"]
        q = e @ old["M"]
        fnd = passed & (q[:, 2] < 0)
        tt = old["b"][2] / np.where(fnd, q[:, 2], -1.0)
        res = np.stack([(q[:, 0] * tt - old["b"][0]) / old["u"] - 0.5, (q[:, 1] * tt - old["b"][1]) / old["v"] - 0.5, np.sqrt((e * e).sum(-1))], -1)
        none = np.stack([X.reshape(-1)[m], Y.reshape(-1)[m], np.zeros(m.sum())], -1).astype(np.float64)
        flat = out.reshape(-1, 3)
        flat[m] = np.where(fnd[:, None], res, none)
        found.reshape(-1)[m] = fnd
        # the margins: a ray EDGE_PX beside the centre that hits where the centre misses (or the other way round), or lands on
        # another layer (t apart by more than 1e-2 of it: a slope of 30 at t = 4.5) -- a silhouette or boundary edge that close; the gate; q.z
        nr = np.zeros(m.sum(), bool)
        for dx, dy in ((EDGE_PX, 0), (-EDGE_PX, 0), (0, EDGE_PX), (0, -EDGE_PX)):
            o2, d2 = object_rays(cs, nodes, i, dx, dy)
            t2, _, _ = closest(v, f, o2[m], d2[m])
            with np.errstate(all="ignore"):
                nr |= (np.isfinite(t2) != hit) | (hit & np.isfinite(t2) & (np.abs(t2 - t) > 1e-2 * np.abs(t)))
        with np.errstate(all="ignore"):
            nr |= hit & (np.abs(rel - depth_tol) < GATE_MARGIN)
            nr |= passed & (np.abs(q[:, 2]) < 1e-3)
        near.reshape(-1)[m] = nr
    return out, found, near


def motion_mesh_px(cam, prev_cam, nodes, prev_nodes, i, v, v_prev, f, z_min):
    """A bound on the float32 error of a mesh pixel's |error of fx| + |error of fy|, by counting operations the way
    test_motion.motion_px does (every operation rounds once, relative error at most 2^-24).  Per component, along the chain of
    k_motion_mesh:
      the camera quantities, the pixel's ray and step 3 (e'.), as counted in test_temporal.delta_px       32
      a'.  per level of the chain p - pos, a 3-term product sum (6), the same for p + d with its sum (7),
           and the difference of the two images (1)                                                        14 L
      b'.  the slot's unit normal as k_mesh_retri left it (6), tri_hit_fin's t: two dot products, a
           difference and the division (12), the hit point p + t d (2)                                     20
           the barycentrics: three tri_area (7 each) with the reciprocal and a product each, c = 1 - a - b 28
      d'.  the combination: three products, two sums                                                        5
           F_i X + t: three products, three sums, and the one rounding of the composed map                  7
    92 + 14 L in all (L = the length of the node's chain).  Like motion_px's, the errors made before the subtraction P_prev - pos'
    are relative to the size of the coordinates they are made in and count relative to z afterwards: the world coordinates |pos|,
    |pos'| and the translations of both chains |t|, and the OBJECT coordinates R of the ray's origin and the mesh (the ray is
    intersected there).  The barycentrics carry the object-space error of the hit point divided by a height of its triangle and
    d'. multiplies it by a previous edge, so those terms grow by kappa = the largest previous edge over the smallest current
    height among the mesh's triangles (at least 1; the deformation's stretch times the triangles' aspect):
      motion_mesh_px = (92 + 14 L) * 2^-24 * (W + H) * kappa * (1 + (|pos| + |pos'| + |t| + R) / z_min)"""
    from tests.test_motion import chain_of
    norm = lambda c: math.sqrt(sum(float(x) ** 2 for x in c.pos))
    L = len(chain_of(nodes, i))
    v, vp = np.asarray(v, np.float64), np.asarray(v_prev, np.float64)
    pn = prev_nodes if prev_nodes is not None else nodes
    t = max(float(np.linalg.norm(from_object(pn, i, np.zeros(3)))), float(np.linalg.norm(from_object(nodes, i, np.zeros(3)))))
    R = float(np.linalg.norm(to_object(nodes, i, np.array(list(cam.pos), np.float64)))) + float(np.abs(v).max()) + float(np.abs(vp).max())
    A, B, C = (v[f[:, k]] for k in range(3))
    area2 = np.linalg.norm(np.cross(B - A, C - A), axis=1)
    longest = np.maximum.reduce([np.linalg.norm(B - A, axis=1), np.linalg.norm(C - B, axis=1), np.linalg.norm(A - C, axis=1)])
    Ap, Bp, Cp = (vp[f[:, k]] for k in range(3))
    longest_prev = np.maximum.reduce([np.linalg.norm(Bp - Ap, axis=1), np.linalg.norm(Cp - Bp, axis=1), np.linalg.norm(Ap - Cp, axis=1)])
    with np.errstate(all="ignore"):
        kappa = max(1.0, float(np.nanmax(longest_prev / (area2 / longest))))
    return (92 + 14 * L) * 2.0 ** -24 * (cam.width + cam.height) * kappa * (1 + (norm(cam) + norm(prev_cam) + t + R) / z_min)
