"""A plain NumPy float32 restatement of the order in which mesh_hit (csrc/rt_trace.h) visits a mesh's four-wide tree
(TEST INFRASTRUCTURE, written from the description of the traversal, not from the kernel's text): per ray the PEAK number
of traversal-stack entries it holds over the whole walk, and the closest triangle it ends on.

Its job is to qualify inputs: a test that is about a deep stack proves with it, before it touches the GPU, that its rays
really reach that depth.  The visiting order decides the occupancy, so every step is the kernel's:

  * the root box (of the reference's own tree: DevMesh::root_box) is tested first;
  * at a node the entry distances of the four children come from the padded slab test -- reciprocal direction, NaN for a
    zero component so that a parallel slab does not constrain, a child entered only if it starts before the closest hit so far;
  * the four (distance, ref) pairs are sorted nearest first by the network (0,1) (2,3) (0,2) (1,3) (1,2), a swap only when the
    second is strictly nearer, so that equal distances keep the child order;
  * the entered children are pushed far to near, the nearest is descended into (nothing entered: pop, or done);
  * a leaf's triangles are tested in slot order with the model's own triangle test in float32 (FIN: two-sided, t > 1e-3; the
    P13 family: back-face culled, bias 1e-7), each accepted hit shrinking the ray; then pop;
  * any_hit: the walk ends at the first leaf that gave a hit.

All rays advance in lock step, one node or one leaf per iteration (the arithmetic is per ray; only the loop is shared)."""
import numpy as np

F = np.float32
LEAF = np.uint32(0x80000000)
DONE = np.uint32(0xFFFFFFFF)
MISS = F(3.0e30)
ENTERED = F(2.0e30)
BIG = F(1.0e30)
MODEL_FIN = 0


def _fmin(a, b):
    return np.fmin(a, b)          # fminf / fmaxf: the operand that is not NaN


def _fmax(a, b):
    return np.fmax(a, b)


def _box_entry(lo, hi, o, inv, zbest):
    """lo, hi, o, inv: (..., 3); zbest: (...).  Entry distance, or MISS."""
    t0, t1 = (lo - o) * inv, (hi - o) * inv
    near, far = _fmin(t0, t1), _fmax(t0, t1)
    tenter = _fmax(_fmax(near[..., 0], near[..., 1]), near[..., 2])
    texit = _fmin(_fmin(far[..., 0], far[..., 1]), far[..., 2])
    hit = (texit >= F(0)) & (tenter <= texit * F(1.000002)) & (tenter * F(0.999998) <= zbest)
    return np.where(hit, tenter, MISS).astype(F)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, p):
    return np.stack([a[..., 1] * p[..., 2] - a[..., 2] * p[..., 1], a[..., 2] * p[..., 0] - a[..., 0] * p[..., 2],
                     a[..., 0] * p[..., 1] - a[..., 1] * p[..., 0]], -1)


def face_normals(v, f):
    """unit face normals as the host computes them for the device triangles: cross(B - A, C - A) / its length, in float32"""
    A, B, C = (v[f[:, k]].astype(F) for k in range(3))
    n = _cross(B - A, C - A)
    with np.errstate(all="ignore"):
        return (n / np.sqrt(_dot(n, n))[:, None]).astype(F)


def _area(ign, A, B, C):
    a0 = (B[:, 1] - A[:, 1]) * (C[:, 2] - A[:, 2]) - (C[:, 1] - A[:, 1]) * (B[:, 2] - A[:, 2])
    a1 = (B[:, 0] - A[:, 0]) * (C[:, 2] - A[:, 2]) - (C[:, 0] - A[:, 0]) * (B[:, 2] - A[:, 2])
    a2 = (B[:, 0] - A[:, 0]) * (C[:, 1] - A[:, 1]) - (C[:, 0] - A[:, 0]) * (B[:, 1] - A[:, 1])
    return np.where(ign == 0, a0, np.where(ign == 1, a1, a2))


def _tri_fin(A, B, C, N, rp, rd, z):
    """the FIN triangle: (accepted, t)"""
    dz = _dot(rd, N)
    pz = _dot(rp - A, N)
    t = -pz / dz
    ok = ~(np.abs(dz) < F(1e-7)) & ~(t <= F(0.001)) & (t < z)
    p = rp + rd * t[:, None]
    ax, ay, az = np.abs(N[:, 0]), np.abs(N[:, 1]), np.abs(N[:, 2])
    ign = np.where((ax > ay) & (ax > az), 0, np.where(ay > az, 1, 2))
    s = F(1) / _area(ign, A, B, C)
    a = _area(ign, p, B, C) * s
    b = _area(ign, p, C, A) * s
    c = F(1) - a - b
    ok &= ~((a < 0) | (b < 0) | (c < 0))
    return ok, t


def _tri_p13(A, B, C, N, rp, rd, z):
    """the P13-family triangle (back-face culled, bias 1e-7): (accepted, t)"""
    bias = F(1e-7)
    ok = ~(_dot(N, rp - A) < bias)
    den = _dot(N, rd)
    ok &= ~(den == 0)
    t = _dot(N, C - rp) / den
    ok &= ~((t < bias) | (t >= z) | (t >= BIG))
    fx, fy, fz = np.abs(N[:, 0]), np.abs(N[:, 1]), np.abs(N[:, 2])
    maxn = _fmax(fz, _fmax(fx, fy))
    P = rp + rd * t[:, None]
    ux = np.where(maxn == fx, 1, 0)                      # the two kept axes: (y, z), (x, z) or (x, y)
    uy = np.where(maxn == fx, 2, np.where(maxn == fy, 2, 1))
    r = np.arange(len(A))
    pax, pay, pbx, pby, pcx, pcy, ppx, ppy = A[r, ux], A[r, uy], B[r, ux], B[r, uy], C[r, ux], C[r, uy], P[r, ux], P[r, uy]
    area_tri = (pax - pcx) * (pby - pcy) - (pay - pcy) * (pbx - pcx)
    area_bcp = (ppx - pcx) * (pby - pcy) - (ppy - pcy) * (pbx - pcx)
    area_acp = (pax - pcx) * (ppy - pcy) - (pay - pcy) * (ppx - pcx)
    alpha, beta = area_bcp / area_tri, area_acp / area_tri
    gam = (1.0 - alpha.astype(np.float64) - beta.astype(np.float64)).astype(F)
    ok &= ~((alpha < -bias) | (beta < -bias) | (gam < -bias) | (alpha > F(1)) | (beta > F(1)) | (gam > F(1)))
    return ok, t


def walk(v, f, nodes, slot_face, root_ref, root_box, rays, model=MODEL_FIN, z0=BIG, any_hit=False):
    """rays (n, 6) float32 in the mesh's own coordinates -> (peak, face, t): per ray the largest number of stack entries held at
    any moment of the traversal, the face it ends on (-1: none) and that hit's distance (z0 where there is none)."""
    rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
    n = len(rays)
    v, f = np.asarray(v, F).reshape(-1, 3), np.asarray(f).reshape(-1, 3)
    tri = v[f[np.asarray(slot_face)]]                    # (slots, 3 corners, 3): the device's triangle slots
    tri_n = face_normals(v, f)[np.asarray(slot_face)]
    lo_all = np.ascontiguousarray(np.transpose(nodes["lo"], (0, 2, 1)), F)      # (node, child, axis)
    hi_all = np.ascontiguousarray(np.transpose(nodes["hi"], (0, 2, 1)), F)
    ref_all = np.asarray(nodes["c"], np.uint32)
    o, d = rays[:, :3].copy(), rays[:, 3:].copy()
    old = np.seterr(all="ignore")
    try:
        inv = np.where(d == 0, F(np.nan), F(1) / d).astype(F)
        z = np.full(n, z0, F)
        root_box = np.asarray(root_box, F)
        entered = _box_entry(root_box[None, :3], root_box[None, 3:], o, inv, z) <= ENTERED
        cur = np.where(entered, np.uint32(root_ref), DONE).astype(np.uint32)
        cap = 16
        stack = np.zeros((n, cap), np.uint32)
        sp = np.zeros(n, np.int64)
        peak = np.zeros(n, np.int64)
        best = np.full(n, -1, np.int64)
        test = _tri_fin if model == MODEL_FIN else _tri_p13

        def pop(idx):
            """rays idx take their next ref off their stacks (DONE where it is empty)"""
            has = sp[idx] > 0
            sp[idx[has]] -= 1
            cur[idx] = np.where(has, stack[idx, np.maximum(sp[idx], 0)], DONE)

        while True:
            active = cur != DONE
            if not active.any():
                break
            inner = np.nonzero(active & ((cur & LEAF) == 0))[0]
            leaf = np.nonzero(active & ((cur & LEAF) != 0))[0]
            if len(inner):
                nd = cur[inner]
                e = _box_entry(lo_all[nd], hi_all[nd], o[inner, None, :], inv[inner, None, :], z[inner, None])      # (k, 4)
                c = ref_all[nd].copy()
                for a, b in ((0, 1), (2, 3), (0, 2), (1, 3), (1, 2)):
                    s = e[:, b] < e[:, a]
                    ea, eb, ca, cb = e[:, a].copy(), e[:, b].copy(), c[:, a].copy(), c[:, b].copy()
                    e[:, a], e[:, b] = np.where(s, eb, ea), np.where(s, ea, eb)
                    c[:, a], c[:, b] = np.where(s, cb, ca), np.where(s, ca, cb)
                if sp[inner].max() + 3 > cap:
                    stack = np.concatenate([stack, np.zeros_like(stack)], 1)
                    cap *= 2
                for k in (3, 2, 1):
                    push = inner[e[:, k] < ENTERED]
                    stack[push, sp[push]] = c[e[:, k] < ENTERED, k]
                    sp[push] += 1
                peak[inner] = np.maximum(peak[inner], sp[inner])
                go = e[:, 0] < ENTERED
                cur[inner[go]] = c[go, 0]
                pop(inner[~go])
            if len(leaf):
                ref = cur[leaf]
                count = ((ref >> np.uint32(28)) & np.uint32(7)).astype(np.int64) + 1
                first = (ref & np.uint32(0x0FFFFFFF)).astype(np.int64)
                got = np.zeros(len(leaf), bool)
                for i in range(4):
                    m = count > i
                    if not m.any():
                        break
                    r, s = leaf[m], first[m] + i
                    ok, t = test(tri[s, 0], tri[s, 1], tri[s, 2], tri_n[s], o[r], d[r], z[r])
                    z[r[ok]] = t[ok]
                    best[r[ok]] = s[ok]
                    got[np.nonzero(m)[0][ok]] = True
                if any_hit:
                    cur[leaf[got]] = DONE
                    leaf = leaf[~got]
                pop(leaf)
    finally:
        np.seterr(**old)
    face = np.where(best >= 0, np.asarray(slot_face, np.int64)[np.maximum(best, 0)], -1)
    return peak, face, z


def through_identity_nodes(rays, positions=((0, 0, 0), (0, 0, 0)), scales=None):
    """the rays as a mesh sees them under nodes that only translate and scale along the axes (by default the root and the mesh's
    own node, both the identity): every level's ToNodeCoords takes the origin as itm * (p - pos) and the direction as
    image(p + d) - image(p), which rounds in float32.  scales: per level the diagonal of the node's tm (itm is its reciprocal;
    the other matrix entries are zero, so every product with them adds an exact zero)."""
    rays = np.array(rays, F).reshape(-1, 6)
    for k, pos in enumerate(positions):
        pos = np.asarray(pos, F)
        itm = F(1) / np.asarray(scales[k] if scales is not None else (1, 1, 1), F)
        p = (rays[:, :3] - pos) * itm
        rays[:, 3:] = ((rays[:, :3] + rays[:, 3:]) - pos) * itm - p
        rays[:, :3] = p
    return rays


def exact_stack_need(nodes, root_ref):
    """the largest number of stack entries ANY ray can hold in this tree: over the root-to-leaf paths, the sum of (children - 1)
    of the nodes on the path.  Also checks that the node refs are in range and that no node is reached twice (a tree)."""
    if int(root_ref) & int(LEAF):
        return 0
    seen = np.zeros(len(nodes), bool)
    worst = 0
    todo = [(int(root_ref), 0)]
    while todo:
        i, held = todo.pop()
        assert 0 <= i < len(nodes), f"node ref {i} out of range"
        assert not seen[i], f"node {i} is reached twice"
        seen[i] = True
        used = ~np.isnan(nodes["lo"][i][0])
        held += int(used.sum()) - 1
        worst = max(worst, held)
        for k in np.nonzero(used)[0]:
            c = int(nodes["c"][i][k])
            if not c & int(LEAF):
                todo.append((c, held))
    assert seen.all(), "a node record is not reachable from the root"
    return worst


def brute_force(v, f, rays, tmin=1e-3):
    """Moeller-Trumbore in float64 over every triangle (two-sided, t > tmin): per ray and face the distance where the ray crosses
    the triangle with barycentrics >= -1e-4 (inf elsewhere), and the same with barycentrics >= +1e-4 -- the faces a float32 test
    MAY accept and the ones it MUST."""
    v, f = np.asarray(v, np.float64).reshape(-1, 3), np.asarray(f).reshape(-1, 3)
    rays = np.asarray(rays, np.float64).reshape(-1, 6)
    A = v[f[:, 0]][None]
    e1, e2 = v[f[:, 1]][None] - A, v[f[:, 2]][None] - A
    may, must = np.empty((len(rays), len(f))), np.empty((len(rays), len(f)))
    step = max(1, 200000 // len(f))                     # a bounded working set whatever the mesh
    for b in range(0, len(rays), step):
        o, d = rays[b:b + step, None, :3], rays[b:b + step, None, 3:]
        with np.errstate(all="ignore"):
            pv = np.cross(d, e2)
            det = (e1 * pv).sum(-1)
            tv = o - A
            u = (tv * pv).sum(-1) / det
            qv = np.cross(tv, e1)
            w = (d * qv).sum(-1) / det
            t = (e2 * qv).sum(-1) / det
            ok = np.isfinite(t) & (t > tmin)
            may[b:b + step] = np.where(ok & (u >= -1e-4) & (w >= -1e-4) & (1 - u - w >= -1e-4), t, np.inf)
            must[b:b + step] = np.where(ok & (u >= 1e-4) & (w >= 1e-4) & (1 - u - w >= 1e-4), t, np.inf)
    return may, must
