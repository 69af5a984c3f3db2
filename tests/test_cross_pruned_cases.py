"""CPU: the premises of the pruned cross sweep's GPU cases (tests/test_gpu_cross_pruned.py, built by
tests/crossprunedref.py) hold -- a case that does not exercise what it names would pass for the wrong reason."""
import numpy as np
import pytest

import crossprunedref as cp
from crossref import F32, bits, block_d2, square


@pytest.fixture(scope="module")
def probe():
    from oracle.oracle import Probe
    return Probe("sse2")


def test_shifted_queries_lie_between_the_blobs():
    Q, R = cp.two_blobs()
    assert Q.shape == (1024, 10) and R.shape == (2048, 10)
    # the reference really is two groups of 1024, 100 apart in column 0
    left = R[:, 0] < 50.0
    assert left.sum() == 1024 and R[left, 0].max() < 1.0 and R[~left, 0].min() > 99.0
    # the unshifted queries sit on the first blob: column 0 alone puts them within r of it, beyond r of the other
    assert np.abs(Q[:, 0]).max() < 1.0
    S = cp.shifted(Q)
    gap0 = np.abs(S[:, None, 0].astype(np.float64) - R[None, :, 0].astype(np.float64))
    assert gap0.min() > 40.0 > cp.BLOB_R    # more than r from EVERY reference frame in column 0 alone
    assert cp.box_gap(S, R[left]) > cp.BLOB_R and cp.box_gap(S, R[~left]) > cp.BLOB_R


@pytest.mark.parametrize("D", [2, 3, 10])
def test_lattice_has_ties_and_the_radii_fall_on_either_side(probe, D):
    g, (r_at, r_above, r_below) = cp.lattice_radii()
    r2 = F32(g * g) * cp.STEP * cp.STEP
    assert square(r_at) == r2
    assert square(r_above) == np.nextafter(r2, F32(np.inf)) and square(r_below) == np.nextafter(r2, F32(0.0))
    for Q, R in (cp.lattice_sets(D, g), cp.lattice_gap_sets(D, g)):
        d2 = block_d2(probe, Q, R)
        ties = bits(d2) == bits(np.full_like(d2, r2))   # canonical d2 bit-equal to r^2
        assert ties.sum() >= 8, (D, int(ties.sum()))
        # strict '<': the ties count for the radius above only; nothing else changes between the three radii
        below, at, above = ((d2 < square(r)).sum() for r in (r_below, r_at, r_above))
        assert below == at and above == at + ties.sum()
    Q, R = cp.lattice_sets(D, g)
    assert len(Q) > 64 and len(R) > 64 and len(Q) % 32 and len(R) % 32   # several tiles, the last one partial
    # the one-tile pair: the boxes are exactly r apart in column 0 (and overlap in column 1)
    Q, R = cp.lattice_gap_sets(D, g)
    assert len(Q) == 32 and len(R) == 32
    assert F32(Q[:, 0].min() - R[:, 0].max()) == F32(r_at) == cp.box_gap(Q, R)
    assert F32(cp.box_gap(Q, R) * cp.box_gap(Q, R)) == r2


def test_degenerate_cases_are_what_they_say(probe):
    cases = {name: (Q, R, radii) for name, Q, R, radii in cp.degenerate_cases()}
    Q, R, _ = cases["one point"]
    assert (R == R[0]).all() and len(R) == 100
    Q, R, radii = cases["one column"]
    assert Q.shape[1] == 3 and (Q[:, :2] == R[0, :2]).all() and (R[:, :2] == R[0, :2]).all()
    assert cp.box_gap(Q, R) == 0 and np.ptp(R[:, 2]) > 1.0
    d2 = block_d2(probe, Q, R)
    assert 0 < (d2 < square(radii[0])).sum() < d2.size
    Q, R, radii = cases["disjoint boxes"]
    assert Q[:, 0].min() > R[:, 0].max()                         # the boxes do not meet ...
    assert 0 < cp.box_gap(Q, R) < F32(radii[0])                  # ... and are closer than r
    assert (block_d2(probe, Q, R) < square(radii[0])).sum() > 0  # pairs across the gap exist
    for name, n_r in (("one query, 64", 64), ("one query, 65", 65)):
        Q, R, _ = cases[name]
        assert len(Q) == 1 and len(R) == n_r
