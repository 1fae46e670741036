"""The photon gather as the ALGORITHM defines it, by brute force (TEST INFRASTRUCTURE: a plain module, no fixtures).

EstimateIrradiance<k> (FIN/include/cyPhotonMap.h:288-336) keeps the k nearest of the photons that lie inside the radius and face the
surface (photonDir.N < 0), and returns their summed power over pi * r_k^2 and the normalised sum of direction * maxPower; r_k^2 is
the k-th smallest squared distance when more than k qualify and radius^2 otherwise.  Here that is one numpy pass per query over all
the photons LocatePhotons can reach: no kd-tree, no heap -- so none of the reference heap's first-replacement quirk -- with every
distance, dot product and sum in float64 from the float32 / byte / int16 photon fields.

Besides the estimate each query gets the figures a test needs to know how far a float32 implementation may sit from it: see Exact."""
import numpy as np

RANK_GAP = 1e-5          # below this relative gap two float32 squared distances may compare either way (fp32 d^2 with contraction is
                         # good to a few ulp, ~4e-7; a traced hit point adds ~1e-6): a factor of ten above both


def reachable(bal):
    """the photons of a balanced 1-based array that LocatePhotons visits: it descends only while index < halfStoredPhotons =
    n/2 - 1 (cyPhotonMap.h:217,371), so heap slots past 2 * half - 1 are never seen"""
    n_stored = len(bal) - 1
    half = n_stored // 2 - 1
    reach = min(max(2 * half - 1, 1), n_stored)
    return bal[1:reach + 1]


def decode(P):
    """(direction (n, 3), power rgb (n, 3)), both float32 exactly as the reference's GetDirection / GetPower return them"""
    f = np.float32
    dx, dy = P["dir_x"].astype(np.int64), P["dir_y"].astype(np.int64)
    z2 = 0x3FFF0001 - np.minimum(dx * dx + dy - dy, 0x3FFF0001)   # GetDirection incl. its dirY - dirY (:158-180)
    dz = np.floor(np.sqrt(z2.astype(np.float64))).astype(np.int64)
    dz = np.where((dz + 1) * (dz + 1) <= z2, dz + 1, dz)
    dz = np.where(dz * dz > z2, dz - 1, dz)
    D = np.stack([dx.astype(f) / f(0x7FFF), dy.astype(f) / f(0x7FFF),
                  np.where(P["plane_and_dirz"] & 8, -1, 1).astype(f) * (dz.astype(f) / f(0x7FFF))], 1)
    power = P["color"].astype(f) / f(255) * P["power"][:, None]
    return D, power


class Exact:
    """per query (arrays of n rows):
    irr[3], dir[3]   the estimate (dir: the normalised sum of direction * maxPower, zero when nothing is accepted)
    M                photons accepted inside the radius
    rk2              r_k^2
    gap              the rank gap (d2[k] - d2[k-1]) / d2[k-1] between the k-th and the (k+1)-th nearest accepted photon; inf when M <= k
    cond             the condition number of the direction sum, sum |term| / |sum term| (1 when nothing is accepted)
    ambiguous        gap < RANK_GAP and the two photons' payloads (power, colour, direction) differ: either may be the k-th
    edge             the smallest |d2 - radius^2| / radius^2 over the facing photons within RANK_GAP of the sphere, where float32
                     may place them on either side; inf without any, or when more than k photons lie safely inside anyway
    facing           the smallest |direction . N| over the photons out to the (k+1)-th distance (the radius when M <= k): near
                     zero the facing test itself may go either way in float32
    sel              (only with keep_sets=True) per query the indices, into reachable(bal), of the photons that count"""

    def __init__(self, n):
        self.irr, self.dir = np.zeros((n, 3)), np.zeros((n, 3))
        self.M = np.zeros(n, np.int64)
        self.rk2, self.gap, self.cond = np.zeros(n), np.full(n, np.inf), np.ones(n)
        self.ambiguous = np.zeros(n, bool)
        self.edge, self.facing = np.full(n, np.inf), np.full(n, np.inf)
        self.sel = None
        self.inputs = None       # (bal, k, r, pos, nrm) in float64, for alternatives()


def gather(bal, k, r, pos, nrm, keep_sets=False, sphere=1.0, edge_on=0.0):
    """Exact for the queries (pos, nrm) against the balanced map `bal`.
    sphere, edge_on: the two decisions float32 may take differently, pushed one way -- a photon is inside when d2 < radius^2 *
    sphere (the area stays pi * radius^2) and faces the surface when direction . N < edge_on (see alternatives())."""
    P = reachable(bal)
    order = np.argsort(P["position"][:, 0], kind="stable")              # sorted by x: a query only looks at the slab its ball lies in
    P = P[order]
    D32, pw32 = decode(P)
    X, D, pw = P["position"].astype(np.float64), D32.astype(np.float64), pw32.astype(np.float64)
    maxp = P["power"].astype(np.float64)
    pay = np.concatenate([D32, pw32, P["power"][:, None]], 1)           # what distinguishes two photons' contributions
    pos, nrm = np.asarray(pos, np.float32).reshape(-1, 3).astype(np.float64), np.asarray(nrm, np.float32).reshape(-1, 3).astype(np.float64)
    r2 = float(np.float32(r) * np.float32(r))                            # the reference squares the radius in float
    ex = Exact(len(pos))
    ex.inputs = (bal, k, r, pos, nrm)
    if keep_sets:
        ex.sel = []
    slab = float(np.float32(r)) * 1.001 + 1e-30                          # a little wider than the ball: edge and facing look just past it
    for i in range(len(pos)):
        lo, hi = np.searchsorted(X[:, 0], [pos[i, 0] - slab, pos[i, 0] + slab])
        d2 = ((X[lo:hi] - pos[i]) ** 2).sum(1)
        dot = D[lo:hi] @ nrm[i]
        faces = ~(dot >= edge_on)
        idx = np.nonzero((d2 < r2 * sphere) & faces)[0]
        # the sphere and the facing test matter only where they can change the set that counts: with more than k photons safely
        # inside, only out to the k-th distance
        on_edge = faces & (np.abs(d2 - r2) < RANK_GAP * r2)
        if on_edge.any() and len(idx) - int((on_edge & (d2 < r2 * sphere)).sum()) <= k:
            ex.edge[i] = np.abs(d2[on_edge] - r2).min() / r2
        reach2 = r2 if len(idx) <= k else min(r2, np.partition(d2[idx], k)[k])
        near = d2 < reach2 * (1 + RANK_GAP)
        if near.any():
            ex.facing[i] = np.abs(dot[near]).min()
        d2 = np.concatenate([np.zeros(lo), d2])                          # indexed like X from here on
        idx += lo
        ex.M[i] = len(idx)
        ex.rk2[i] = r2
        if len(idx) > k:
            part = idx[np.argpartition(d2[idx], k)[:k + 1]]              # the k + 1 nearest, then in order
            part = part[np.argsort(d2[part], kind="stable")]
            a, b = part[k - 1], part[k]
            ex.rk2[i] = d2[a]
            ex.gap[i] = (d2[b] - d2[a]) / d2[a] if d2[a] > 0 else (0.0 if d2[b] == d2[a] else np.inf)
            ex.ambiguous[i] = ex.gap[i] < RANK_GAP and not (pay[a] == pay[b]).all()
            idx = part[:k]
        if keep_sets:
            ex.sel.append(order[idx])
        if len(idx) == 0:
            continue
        ex.irr[i] = pw[idx].sum(0) / (np.pi * ex.rk2[i]) if ex.rk2[i] > 0 else pw[idx].sum(0)
        terms = D[idx] * maxp[idx, None]
        tot = terms.sum(0)
        norm = np.linalg.norm(tot)
        if norm > 0:
            ex.dir[i] = tot / norm
            ex.cond[i] = np.linalg.norm(terms, axis=1).sum() / norm
    return ex


def irradiance_error(irr, ex):
    """per query: the largest channel difference relative to the query's largest channel (the project's bar for it: 2e-5)"""
    scale = np.abs(ex.irr).max(axis=1) + 1e-30
    return np.abs(np.asarray(irr, np.float64) - ex.irr).max(axis=1) / scale


def alternatives(ex, rows):
    """The estimates of the queries `rows` under every way float32 may decide what float64 cannot tell it: a photon within
    RANK_GAP of the sphere counted as inside or as outside, a photon edge-on to the surface (|direction . N| < 1e-6) counted as
    facing it or not -- all such photons of a query one way together, which covers the single photon there is in practice."""
    bal, k, r, pos, nrm = ex.inputs
    return [gather(bal, k, r, pos[rows], nrm[rows], sphere=sp, edge_on=eo)
            for sp in (1 - 2 * RANK_GAP, 1 + 2 * RANK_GAP) for eo in (-2e-6, 2e-6)]


def assert_matches(irr, ex, k, what, direction=None, max_loose=0.02):
    """Every query against the brute force: 2e-5 of its largest channel (direction: 2e-5 * cond absolute).  A query that is
    ambiguous in rank (the k-th and the (k+1)-th photon closer than RANK_GAP in d^2, with different payloads) is held to one
    photon's worth, 2.5 / k + 2e-5, and at most max_loose of the queries may be.  A query with a photon ON the sphere or edge-on to
    the surface (Exact.edge, Exact.facing) has two legitimate answers, with that photon and without it: it must match one of
    them (alternatives()) at the same 2e-5.  Which rows are zero must agree exactly."""
    irr = np.asarray(irr, np.float64)
    rel = irradiance_error(irr, ex)
    either = np.nonzero((ex.edge < RANK_GAP) | (ex.facing < 1e-6))[0]
    if len(either):
        alts = alternatives(ex, either)
        best = np.min([irradiance_error(irr[either], a) for a in alts], axis=0)
        amb_any = np.any([a.ambiguous for a in alts], axis=0)
        assert (best[~amb_any] < 2e-5).all(), (what, "queries with a photon on the sphere or edge-on", either, best)
        assert (best[amb_any] < 2.5 / k + 2e-5).all(), (what, either, best)
    decided = np.ones(len(rel), bool)
    decided[either] = False
    amb = ex.ambiguous & decided
    tight = decided & ~amb
    assert amb.mean() <= max_loose, (what, int(amb.sum()), len(rel))
    assert (rel[tight] < 2e-5).all(), (what, "worst", rel[tight].max(), "query", int(np.argmax(np.where(tight, rel, 0))))
    assert (rel[amb] < 2.5 / k + 2e-5).all(), (what, rel[amb])
    assert ((irr == 0).all(axis=1) == (ex.irr == 0).all(axis=1))[tight].all(), what
    if direction is not None:
        dd = np.abs(np.asarray(direction, np.float64) - ex.dir).max(axis=1)
        assert (dd[tight] <= 2e-5 * ex.cond[tight]).all(), (what, "direction", dd[tight].max())
    return rel
