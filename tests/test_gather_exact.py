"""tests/gather_exact.py (the brute-force float64 k-nearest gather the GPU tests compare with) against the REFERENCE's own
EstimateIrradiance<k> outputs in the golden vectors: no GPU needed."""
import numpy as np
import pytest

from tests import gather_exact


@pytest.mark.parametrize("tag", ["k50", "k400"])
def test_brute_force_gather_agrees_with_the_reference_vectors(gold, tag):
    """The reference's heap drops its farthest photon on the first replacement even when the newcomer is farther
    (cyPhotonMap.h:424-436), so some of its queries end with the (k+1)-th nearest photon instead of the k-th: an O(1/k)
    difference.  The allowance is the one the GPU tests give that quirk: at least 90 % of the queries within 2e-5 of their
    largest channel, the rest within 2.5 / k + 1e-4; directions of the tight queries within 2e-5 * cond."""
    g = gold(f"photon_{tag}.npz")
    k, radius = int(g["k"]), float(g["radius"])
    q, ref = g["queries"], g["result"]
    ex = gather_exact.gather(g["balanced"], k, radius, q[:, :3], q[:, 3:])
    rel = gather_exact.irradiance_error(ref[:, :3], ex)
    tight = rel < 2e-5
    assert tight.mean() >= 0.9, rel
    assert (rel[~tight] < 2.5 / k + 1e-4).all(), rel[~tight]
    assert ((ref[:, :3] == 0).all(axis=1) == (ex.irr == 0).all(axis=1)).all()
    dd = np.abs(ref[:, 3:] - ex.dir).max(axis=1)
    assert (dd[tight] <= 2e-5 * ex.cond[tight]).all(), dd[tight].max()
    # the figures that go with the estimate
    assert (ex.M > 0).mean() > 0.5 and (ex.M > k).any()
    assert ((ex.M > k) == np.isfinite(ex.gap)).all() and (ex.gap >= 0).all()
    r2 = float(np.float32(radius) * np.float32(radius))
    assert (ex.rk2[ex.M <= k] == r2).all() and (ex.rk2[ex.M > k] < r2).all()
    assert (ex.cond >= 1 - 1e-12).all()


def test_brute_force_gather_on_a_hand_made_map():
    """five photons on a line, one of them travelling away from the surface: counts, r_k^2, the rank gap and the sums by hand"""
    from raytracing_folder_amd import capi
    ph = np.zeros(6, capi.PHOTON)
    for i, x in enumerate([1.0, 2.0, 3.0, 4.0, 1.5]):
        ph[i + 1]["position"] = (x, 0, 0)
        ph[i + 1]["power"] = 2.0
        ph[i + 1]["color"] = (255, 51, 0)
        ph[i + 1]["plane_and_dirz"] = 8                    # direction (0, 0, -1)
    ph[5]["plane_and_dirz"] = 0                            # the photon at 1.5 travels the other way: rejected
    # the brute force reads no tree, only the prefix rule: 45 stored photons, half = 21, the first 41 are reachable
    far = np.zeros(40, capi.PHOTON)
    far["position"] = (1000, 0, 0)
    far["plane_and_dirz"] = 8
    bal = np.concatenate([ph, far])
    assert len(gather_exact.reachable(bal)) == 41
    ex = gather_exact.gather(bal, 3, 10.0, [[0, 0, 0]], [[0, 0, 1]], keep_sets=True)
    assert ex.M[0] == 4 and ex.rk2[0] == 9.0 and ex.gap[0] == pytest.approx((16 - 9) / 9)
    assert sorted(bal[1:]["position"][ex.sel[0], 0]) == [1.0, 2.0, 3.0]
    assert ex.irr[0] == pytest.approx(np.array([6.0, 6.0 * float(np.float32(51) / np.float32(255)), 0]) / (np.pi * 9.0))
    assert (ex.dir[0] == (0, 0, -1)).all() and ex.cond[0] == pytest.approx(1.0) and not ex.ambiguous[0]
    ex = gather_exact.gather(bal, 4, 10.0, [[0, 0, 0]], [[0, 0, 1]])
    assert ex.M[0] == 4 and ex.rk2[0] == 100.0 and np.isinf(ex.gap[0])
    ex = gather_exact.gather(bal, 4, 10.0, [[0, 0, 0]], [[0, 0, -1]])
    assert ex.M[0] == 1 and (ex.dir[0] == (0, 0, 1)).all()            # only the one that was rejected before
