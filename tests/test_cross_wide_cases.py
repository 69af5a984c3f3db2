"""CPU: the case generators of the cross-wide sweeps' tests (tests/crosswideref.py) really hold what the GPU tests
(tests/test_gpu_cross_wide.py) rely on, against the probe and in every summation order: pairs exactly on fl32(r^2) and
one ulp to either side ACROSS the two sets, equal-distance references at scattered indices, duplicates between Q and R
and inside R, data that trips the statistics flag in one set only, and blob sets whose pairs almost all lie clear of the
kernel's band -- the band of Q and R stacked, since the statistics of a cross sweep run over both."""
import numpy as np
import pytest

import crossref
import crosswideref as cw
import wideref

F32 = np.float32
ORDERS = ("sse2", "avx", "fma")


def d2_block(order, Q, R):
    from oracle.oracle import Probe
    return crossref.block_d2(Probe(order), Q, R)


@pytest.mark.parametrize("n_q,n_r,n_cols", [(300, 300, 80), (130, 200, 65), (40, 2100, 256)])
def test_boundary_sets_hold_pairs_on_the_radius_and_one_ulp_to_either_side(oracle, n_q, n_r, n_cols):
    Q, R, r, groups = cw.boundary_sets(n_q, n_r, n_cols)
    r2 = crossref.square(r)
    assert r2 == F32(9.0) and len(groups) == 3
    for order in ORDERS:
        d2 = d2_block(order, Q, R)
        for a, b, c, d in groups:
            assert len({b // 32, c // 32, d // 32}) == 3, "the reference rows of a group in different tiles"
            assert d2[a, b] == r2, (order, a, b)
            assert d2[a, c] == np.nextafter(r2, F32(np.inf)), (order, a, c)
            assert d2[a, d] == np.nextafter(r2, F32(0)), (order, a, d)
        # the strict comparison: of the three only the pair an ulp inside counts
        pops = crossref.expect_pops(d2, [r])[0]
        for a, b, c, d in groups:
            others = np.delete(d2[a], [b, c, d])
            assert pops[a] == 1 + int((others < r2).sum())
    # the groups use nine different reference rows and three different queries
    assert len({j for g in groups for j in g[1:]}) == 9 and len({g[0] for g in groups}) == 3


@pytest.mark.parametrize("n_q,n_r,n_cols", [(130, 200, 129), (300, 300, 80)])
def test_ties_sets_hold_equal_distances_and_duplicates(n_q, n_r, n_cols):
    Q, R, stars, copies, twins = cw.ties_sets(n_q, n_r, n_cols)
    for order in ORDERS:
        d2 = d2_block(order, Q, R)
        nn_i, nn_d = crossref.expect_nn(d2)
        for q, ring in stars:
            assert [d2[q, j] for j in ring] == [F32(2.0 ** -12)] * 4, (order, q)
            assert int((d2[q] == d2[q].min()).sum()) == 4 and d2[q].min() == F32(2.0 ** -12), "nothing else as close"
            assert nn_i[q] == min(ring) and min(ring) != ring[0] and sorted(ring) != ring, "the ring is not met in index order"
        for q, j in copies:
            assert (Q[q] == R[j]).all() and d2[q, j] == 0 and int((d2[q] == 0).sum()) == 1 and nn_i[q] == j
        for q, lo, hi in twins:
            assert lo < hi and (R[lo] == R[hi]).all() and d2[q, lo] == 0 and d2[q, hi] == 0 and nn_i[q] == lo


def test_flagged_sets_trip_the_flag_in_one_set_only():
    Q, R = cw.blob_sets(100, 130, 200)
    assert not crossref.stats_flagged(Q, R)
    for flaw in cw.FLAWS:
        Qf, Rf = cw.flawed_sets(Q, R, flaw)
        assert crossref.stats_flagged(Qf, Rf), flaw
        clean_q, clean_r = np.isfinite(Qf).all() and (Qf == Q).all(), np.isfinite(Rf).all() and (Rf == R).all()
        assert clean_q != clean_r, (flaw, "one set stays as it was")
    # the far-apart sets of the offset case are finite and far below the limit: the matrix-core kernel answers them
    Qo, Ro = cw.offset_sets(100, 130, 200)
    assert not crossref.stats_flagged(Qo, Ro)


@pytest.mark.parametrize("n_cols", [65, 256])
def test_blob_sets_keep_their_pairs_clear_of_the_band(n_cols):
    """the share of (query, reference) pairs within 2 eps of a threshold (radii at the 25 % and 5 % quantiles of d2) stays
    under 1 %, eps being the band of the kernel for Q and R stacked"""
    Q, R = cw.blob_sets(n_cols, 1500, 1500)
    both = np.vstack([Q, R])
    q, r = Q.astype(np.float64), R.astype(np.float64)
    d2 = np.maximum((q * q).sum(axis=1)[:, None] + (r * r).sum(axis=1)[None, :] - 2.0 * (q @ r.T), 0.0).ravel()
    for quant in (0.25, 0.05):
        r2 = float(np.quantile(d2, quant))
        e = wideref.eps(n_cols, both, r2)
        share = float((np.abs(d2 - r2) < 2.0 * e).mean())
        print(f"D={n_cols} quantile {quant}: r2={r2:.4f} eps={e:.3e} share within 2 eps = {100 * share:.4f} %")
        assert e > 0 and share < 0.01, (n_cols, quant, share)
    assert len(np.unique(both, axis=0)) == len(both), "no frame twice: a duplicate pair is a legitimate candidate"


def test_offset_sets_have_no_partners_and_far_neighbours():
    Q, R = cw.offset_sets(100, 130, 200)
    d2 = d2_block("sse2", Q, R)
    radii = cw.radii_for(100, 3)
    assert int(crossref.expect_pops(d2, radii).sum()) == 0
    assert float(d2.min()) > 4.0 * max(radii) ** 2
