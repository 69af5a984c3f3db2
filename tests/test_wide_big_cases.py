"""CPU: what tests/test_gpu_wide_big.py relies on.  The unit map of the wide matrix-core sweeps -- wide_shares, wide_unit
and wide_grid_size of dc_mfma_wide_kernels.hpp, through the host-only modes of clustering_amd/bin/test_wide_model -- meets
every (query block, share) exactly once at every share count and on both sides of every launch group, and keeps the
locality its comment claims; and the case generators of tests/widebigref.py hold their conditions against the oracles
in every summation order."""
import numpy as np
import pytest

import crossref
import wideref
import widebigref as wb

F32 = np.float32
ORDERS = ("sse2", "avx", "fma")
SHARE_COUNTS = (1, 2, 4, 8, 16, 32, 64)
QUERY_BLOCKS = (1, 7, 8, 9, 16, 17, 65, 513, 1030)


def test_share_counts_at_every_seam():
    want = [(15, 1), (16, 2), (31, 2), (32, 4), (63, 4), (64, 8), (127, 8), (128, 16), (255, 16), (256, 32), (511, 32),
            (512, 64), (513, 64), (4000, 64)]
    assert [(rb, wb.shares(rb)) for rb, _ in want] == want


@pytest.mark.parametrize("n_shares", SHARE_COUNTS)
def test_every_query_block_meets_every_share_exactly_once(n_shares):
    for qb in QUERY_BLOCKS:
        grid, tab = wb.units(n_shares, qb)
        assert grid > 0 and grid % wb.GROUP == 0, (n_shares, qb, grid)
        assert (tab[:, 1] < n_shares).all()
        inside = tab[:, 0] < qb
        met = np.zeros((qb, n_shares), dtype=np.int64)
        np.add.at(met, (tab[inside, 0], tab[inside, 1]), 1)
        assert (met == 1).all(), (n_shares, qb, "unanswered" if (met == 0).any() else "answered twice", np.argwhere(met != 1)[:4])
        # every other workgroup pads the last group: a query block past the end, which the kernel leaves at once
        assert int(inside.sum()) == qb * n_shares and (tab[~inside, 0] >= qb).all()


@pytest.mark.parametrize("n_shares", [s for s in SHARE_COUNTS if s >= 8])
def test_an_xcd_runs_eight_query_blocks_by_eight_shares_side_by_side(n_shares):
    """workgroups go round-robin to the 8 XCDs by their id: every run of 64 consecutive workgroups of one XCD is 8 query
    blocks x 8 shares, and with 64 shares XCD x only ever meets the shares 8 x .. 8 x + 7"""
    for qb in (9, 65, 513):
        grid, tab = wb.units(n_shares, qb)
        for xcd in range(8):
            mine = tab[xcd::8]
            assert len(mine) % 64 == 0
            for a in range(0, len(mine), 64):
                run = mine[a:a + 64]
                qs, ss = set(run[:, 0].tolist()), set(run[:, 1].tolist())
                assert len(qs) == 8 and len(ss) == 8 and len({(q, s) for q, s in run.tolist()}) == 64, (n_shares, qb, xcd, a)
            if n_shares == 64:
                assert set(mine[:, 1].tolist()) == set(range(8 * xcd, 8 * xcd + 8)), (qb, xcd)


@pytest.mark.parametrize("n_shares", [1, 2, 4])
def test_with_fewer_than_eight_shares_an_xcd_runs_every_share_of_further_query_blocks(n_shares):
    grid, tab = wb.units(n_shares, 513)
    for xcd in range(8):
        mine = tab[xcd::8]
        for a in range(0, len(mine), 64):
            run = mine[a:a + 64]
            assert len(set(run[:, 1].tolist())) == n_shares and len(set(run[:, 0].tolist())) == 64 // n_shares


@pytest.mark.parametrize("R_rows,n_shares", [(8192, 8), (65664, 64)])
@pytest.mark.parametrize("self_form", [False, True])
def test_star_rows_lie_in_the_shares_waves_and_halves_they_are_meant_for(R_rows, n_shares, self_form):
    from oracle.oracle import Oracle
    case = wb.star_across_shares(R_rows, 65, n_shares, self_form=self_form)
    R, S = case["R"], n_shares
    assert wb.shares_of_rows(R_rows) == S, "the share count the product picks for this reference"
    oracles = [Oracle(order=o) for o in ORDERS]
    for k, (centre, ring, fe_c) in enumerate(case["stars"]):
        a, b, c, d, e, f = ring
        pa, pb, pc, pd, pe, pf = (wb.place(r, S) for r in ring)
        assert a == min(ring), "the lowest index"
        assert pa[:3] == pb[:3] and a // 32 == b // 32 and (pa[3], pb[3]) == (0, 1), "one tile, the two halves of a wave"
        reg = lambda row: ((row % 32) & 3) + 4 * ((row % 32) >> 3)   # (tile_row_local, inverted)
        assert reg(b) < reg(a), "b sits in a lower accumulator register of its lane: the wave meets it before a"
        assert pa[0] == pc[0] and (pa[2], pc[2]) == (0, 1), "one block, the other pair of waves"
        assert pa[1] == pd[1] and pa[0] != pd[0], "one share, another block"
        assert len({pa[1], pe[1], pf[1]}) == 3, "three different shares"
        for o in oracles:
            dist = [o.dist2(centre, R[r]) for r in ring] + [o.dist2(R[r], centre) for r in ring]
            assert all(x == wb.TIE_D2 for x in dist), (k, dist)
        fr = case["fe_r"][ring]
        if k == 0:
            assert (fr < fe_c).all()
        else:
            assert (fr[:4] > fe_c).all() and (fr[4:] < fe_c).all() and e == min(e, f) and pe[1] != pa[1], "nn and nn_hd in different shares"
    vec, lo, hi, fe_c = case["dup"]
    assert lo < hi and (R[lo] == R[hi]).all() and (R[lo] == vec).all() and wb.place(lo, S)[1] != wb.place(hi, S)[1]
    # nothing else is as close: the nearest other row of every centre lies beyond the ring
    centres = np.vstack([s[0] for s in case["stars"]] + [vec])
    from oracle.oracle import Probe
    d2 = wb.rect_d2(Probe(), centres, R)
    special = [set(s[1]) for s in case["stars"]] + [{lo, hi}]
    own = case.get("centres", [None] * 3)
    for k in range(3):
        others = np.delete(d2[k], sorted(special[k] | ({own[k]} if self_form else set())))
        assert float(others.min()) > 64 * float(wb.TIE_D2), (k, float(others.min()))
        assert (d2[k, sorted(special[k])] == (0 if k == 2 else wb.TIE_D2)).all()
    if self_form:
        lo_, hi_ = case["span"]
        assert all(lo_ <= r < hi_ for r in own) and hi_ <= R_rows and len({r // 128 for r in own}) == 3
        for k, row in enumerate(own):
            assert (R[row] == centres[k]).all()


@pytest.mark.parametrize("n_cols", [65, 256])
def test_outlier_case_puts_every_cluster_pair_inside_the_band_of_every_radius(n_cols):
    case = wb.outlier_case(500, n_cols)
    c, radii, n = case["c"], case["radii"], case["n_cluster"]
    assert len(radii) == 8 and len(set(radii)) == 8 and sorted(radii) != radii
    assert not crossref.stats_flagged(c[:1], c[1:]) and not crossref.stats_flagged(case["Q"], case["R"])
    assert sorted(map(tuple, np.vstack([case["Q"], case["R"]]))) == sorted(map(tuple, c)), "the cross split holds the same rows"
    m = wb.extent(c)
    assert 0.99 * wb.OUTLIER_L ** 2 < m < 1.01 * wb.OUTLIER_L ** 2, "the two far rows set the scale"
    from oracle.oracle import Probe
    d2 = Probe().pairwise_d2(c)
    iu = np.triu_indices(n, 1)
    pairs = d2[:n, :n][iu].astype(np.float64)
    far = d2[n:, :n].astype(np.float64)
    for r in radii:
        r2 = float(crossref.square(r))
        e = wideref.eps(n_cols, c, r2)
        worst = float(np.abs(pairs - r2).max())
        print(f"D={n_cols} r2={r2:.5f}: eps={e:.4f}, cluster pairs within {worst:.4f} of it, {int((pairs < r2).sum())} inside")
        assert worst <= e / 2, (n_cols, r, worst, e)
        assert float(far.min()) > r2 + 2 * e and float(d2[n, n + 1]) > r2 + 2 * e
    inside = [int((pairs < float(crossref.square(r))).sum()) for r in radii]
    assert len(set(inside)) == 8 and min(inside) > 0 and max(inside) < len(pairs), "the exact decisions differ from radius to radius"


@pytest.mark.parametrize("one_ulp", [False, True])
def test_identical_rows_have_no_extent_and_their_expected_results(oracle, one_ulp):
    n, d = 300, 100
    c = wb.identical_rows(n, d, one_ulp)
    norm = float((c[0].astype(np.float64) ** 2).sum())
    m = wb.extent(c)
    assert m <= 4 * 2.0 ** -46 * norm, (m, norm)
    assert (m == 0) == (not one_ulp)
    assert not crossref.stats_flagged(c[:1], c[1:])
    pops = oracle.populations(c, wb.DEGENERATE_RADII)
    fe = wb.fe_random(n)
    nn = oracle.nearest_neighbors(c, fe)
    r2 = [crossref.square(r) for r in wb.DEGENERATE_RADII]
    assert r2[0] == 0 and r2[1] == 0 and np.isinf(r2[5]) and r2[4] < np.inf, "1e-30 squares to 0 in float: it is radius 0"
    for k in range(len(r2)):
        assert (pops[k] == (n if r2[k] > 0 else 1)).all(), k   # (d2 < 0 holds for nothing: the frame's own 1)
    if not one_ulp:
        assert int(nn[0][0]) == 1 and (nn[0][1:] == 0).all() and (nn[1] == 0).all()
    else:
        odd = n // 2 + 3
        assert 0 < nn[1][odd] < 1e-12 and int(nn[0][odd]) == 0 and nn[1][0] == 0 and int(nn[0][0]) == 1


def test_rect_d2_is_the_block_of_the_union(probe):
    Q, R = crossref.sets(65, 150, 333, seed=3)
    want = crossref.block_d2(probe, Q, R)
    for chunk in (64, 100, 1024):
        assert (crossref.bits(wb.rect_d2(probe, Q, R, chunk)) == crossref.bits(want)).all(), chunk
