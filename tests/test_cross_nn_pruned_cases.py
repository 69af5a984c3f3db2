"""CPU: the premises of the built cases of tests/test_gpu_cross_nn_pruned.py (tests/crossnnref.py), from the probe's
canonical d2 alone."""
import numpy as np
import pytest

import crossnnref as cn
import crossprunedref as cp
from crossref import F32, FLT_MAX, block_d2, expect_nn


@pytest.fixture(scope="module")
def probe():
    from clustering_amd import capi
    from oracle.oracle import Probe
    return Probe(capi.CANON_ORDER)


def test_who_answered_premise(probe):
    """every query has a lower-energy reference in its own blob, and no ring can reach the other blob: a ring grows to
    at most 4 x 1.001 x the largest exact incumbent, far below the squared gap between the blobs"""
    Q, R, fe_q, fe_r = cn.who_answered()
    d2 = block_d2(probe, Q, R)
    own = cn.own_blob(R)
    assert own.sum() == cp.BLOB_ROWS
    nn_i, nn_d, hd_i, hd_d = expect_nn(d2, fe_q, fe_r)
    assert own[hd_i].all() and own[nn_i].all() and (hd_d < FLT_MAX).all()
    gap = float(R[~own, 0].min() - max(R[own, 0].max(), Q[:, 0].max()))
    # a ring ends at most at 4 x 1.001 x (the largest of: the exact incumbents, the first ring's end); the first ring ends
    # at max(extent^2 of a query group -- at most that of all queries --, cell^2, gap to R's box = 0)
    cell, _ = cn.cell_order(Q, R)
    ext2 = float(np.ptp(Q[:, 0])) ** 2 + float(np.ptp(Q[:, 1])) ** 2
    widest = max(float(hd_d.max()), float(cell) ** 2, ext2)
    assert 4.0 * 1.001 * widest < 1e-3 * gap * gap, (hd_d.max(), cell, ext2, gap)
    # the cap of the GPU test: 32 tiles of the own blob + 1 straddling of 64, times the padding of the last query group
    T_q = (len(Q) + 31) // 32
    pad = (-(-T_q // cn.TQ_BUILT) * cn.TQ_BUILT) / T_q
    assert 33 / 64 * pad <= 0.75


@pytest.mark.parametrize("D", [2, 3, 10])
def test_tie_geometry(probe, D):
    """the tie of case 3 (a) and the rings in which the sweep meets its two tiles (crossnnref.tie_sets)"""
    Q, R = cn.tie_sets(D)
    d2 = block_d2(probe, Q, R)
    want = cn.TIE_D2
    assert (d2[:, :64] == want).all() and (d2[:, 64:] > want).all()   # 64 references at exactly the same distance
    # the rings, restated: the first ends at max(group extent^2 = 0, cell^2, gap to R's box = 0), an empty one is
    # followed by one four times as wide
    cell, order = cn.cell_order(Q, R)
    first = F32(cell) * F32(cell)
    assert first == F32(6.25) and first < want and F32(4.0) * first == want
    assert cp.box_gap(Q, R) == 0.0
    # tile 0 of the order: the far rows alone, a box of one point whose gap IS the tie distance (not inside a ring that
    # ends there); tile 1: the near rows alone, nearer; every other tile farther than the first ring's end, so that
    # ring is empty
    assert sorted(order[:32]) == list(range(32)) and sorted(order[32:64]) == list(range(32, 64))
    assert cp.box_gap(Q, R[order[:32]]) ** 2 == want
    assert first <= cp.box_gap(Q, R[order[32:64]]) ** 2 == F32(9.0) < want
    for t in range(2, len(R) // 32):
        assert cp.box_gap(Q, R[order[32 * t:32 * t + 32]]) ** 2 > want
    # so after the ring that ends at 25 every incumbent is (25, index >= 32); the answer is in the far tile
    fe_q, fe_r = cn.tie_fe(len(Q), len(R))
    nn_i, _, hd_i, hd_d = expect_nn(d2, fe_q, fe_r)
    assert (nn_i == 0).all() and (hd_i == 3).all() and (hd_d == want).all()


def test_far_lower_premise(probe):
    Q, R, fe_q, fe_r, special = cn.far_lower()
    d2 = block_d2(probe, Q, R)
    _, _, hd_i, hd_d = expect_nn(d2, fe_q, fe_r)
    near = R[:, 0] < 50.0
    assert not near[special]
    low = fe_q == F32(0.5)
    assert low.sum() == 40 and (fe_r[near].min() > F32(0.5)) and ((fe_r < F32(0.5)).sum() == 1)
    assert (hd_i[low] == special).all() and (hd_d[low] > 90.0 ** 2).all()     # the only lower frame is in the other blob
    assert near[hd_i[~low]].all()


def test_numpy_float32_is_the_canonical_d2_in_one_column(probe):
    rng = np.random.default_rng(10)
    q = rng.normal(size=(32, 1)).astype(np.float32)
    r = rng.normal(size=(4096, 1)).astype(np.float32)
    d2 = block_d2(probe, q, r)
    diff = (q - r.T).astype(np.float32)
    assert (d2.view(np.uint32) == (diff * diff).astype(np.float32).view(np.uint32)).all()
