"""CPU: the premises of the GPU cases of the radius graph at 257..1024 columns (tests/xwidegraphref.py), with a numpy cell
order and the probe's canonical d2: the stretched blobs drop block pairs at the graph's radius (the lower bound of the
counter lies below all tile pairs), the boundary case has pairs on the radius and one ulp to either side of it in the
canonical arithmetic, the duplicated rows of the small-radius case are its only pairs, and the min-edge case has 6 blocks.
The block-pair bounds the GPU counters are held to (xwidegraphref.tile_bounds_r2) are computed here under that order."""
import numpy as np
import pytest

import graphref
import widegraphpruneref as wgp
import widegraphref as wg
import widepruneref as pr
import xwidegraphref as xg
import xwidepruneref as xp

F32 = np.float32


@pytest.mark.parametrize("n_cols", xg.TABLE_COLS)
@pytest.mark.parametrize("n_rows", xg.STRETCHED_ROWS)
def test_the_stretched_blobs_drop_block_pairs_at_the_graphs_radius(n_rows, n_cols):
    c, r, r2 = xg.stretched_case(n_rows, n_cols)
    assert r == max(xp.radii_for(n_cols)) and r2 == F32(F32(r) * F32(r))
    assert [float(r2)] == pr.launch_r2max(xp.radii_for(n_cols)), "the radius the population table was made for"
    perm = pr.cell_order(c)
    assert not np.array_equal(perm, np.arange(n_rows)), "the order is not the identity"
    nb = pr.n_blocks(n_rows)
    lo, hi = xg.tile_bounds_r2(c, perm, r2)
    print(f"{n_rows} x {n_cols}: tile pairs in [{lo}, {hi}] of {xg.all_tiles(n_rows)}")
    assert (lo // 16, nb * nb) == xp.POP_TABLE[n_rows] and lo == hi
    assert 16 * nb <= lo < xg.all_tiles(n_rows), "every block meets itself; lower < all: block pairs are dropped"
    parts = [xg.tile_bounds_r2(c, perm, r2, s, 3) for s in range(3)]
    assert tuple(map(sum, zip(*parts))) == (lo, hi), "the bounds of three segments add up"
    if n_rows > 700:
        turned = wgp.pairs_against_the_order(wgp.pairs_float64(c, r2), perm)
        assert len(turned) > 100, "pairs whose rows stand the other way round in the order"


def test_block_counts_and_shares_of_the_shapes():
    assert [pr.n_blocks(n) for n in xg.STRETCHED_ROWS] == [6, 12, 17]
    assert [pr.shares(pr.n_blocks(n)) for n in xg.STRETCHED_ROWS] == [1, 1, 2]
    assert pr.n_blocks(xg.SMALL_RADIUS_SHAPE[0]) == 65 and pr.n_blocks(xg.BOUNDARY_SHAPE[0]) == 3


def test_the_boundary_case_has_pairs_on_and_one_ulp_to_either_side_of_the_radius(probe):
    c, r, r2, groups = xg.boundary_case()
    assert c.shape == xg.BOUNDARY_SHAPE and r2 == F32(9.0)
    d2 = probe.pairwise_d2(c)
    below, above = np.nextafter(F32(9.0), F32(0.0)), np.nextafter(F32(9.0), F32(np.inf))
    assert len(groups) == 3
    for a, b, cc, d in groups:
        assert d2[a, b] == F32(9.0) and d2[b, a] == F32(9.0), "on the radius: outside"
        assert d2[a, cc] == above, "one ulp outside"
        assert d2[a, d] == below, "one ulp inside"
    want = graphref.pairs_of(d2, r2)
    got = set(graphref.keys(want, len(c)).tolist())
    for a, b, cc, d in groups:
        assert int(graphref.keys([[a, d]], len(c))[0]) in got
        assert int(graphref.keys([[a, b]], len(c))[0]) not in got and int(graphref.keys([[a, cc]], len(c))[0]) not in got
    lo, hi = xg.tile_bounds_r2(c, pr.cell_order(c), r2)
    assert lo == hi == xg.all_tiles(len(c)), "blobs of sigma 0.3 at r = 3: nothing to prune"


def test_the_duplicated_rows_of_the_small_radius_case_are_its_only_pairs(probe):
    c, r, r2, dups = xg.small_radius_case()
    assert c.shape == xg.SMALL_RADIUS_SHAPE
    assert len(dups) == 24 and len(np.unique(dups)) == 48 and (c[dups[:, 0]] == c[dups[:, 1]]).all()
    n = len(c)
    want = graphref.brute_pairs(probe, c, r2)
    assert np.array_equal(np.sort(graphref.keys(want, n)), np.sort(graphref.keys(dups, n)))
    perm = pr.cell_order(c)
    empty, units = pr.empty_units(c, perm, float(r2))
    assert units == 8 * 65 and empty > 0, "(query block, share) units without a survivor"
    lo, hi = xg.tile_bounds_r2(c, perm, r2)
    assert 16 * 65 <= lo <= hi < xg.all_tiles(n)


def test_the_min_edge_case_has_six_blocks_tied_partners_and_both_rank_branches():
    c, r, r2, dups = xg.min_edge_case()
    assert c.shape == xg.MIN_EDGE_SHAPE and (c[dups[:, 0]] == c[dups[:, 1]]).all()
    n = len(c)
    assert pr.n_blocks(n) == 6
    perm = pr.cell_order(c)
    lo, hi = xg.tile_bounds_r2(c, perm, r2)
    assert 16 * 6 <= lo == hi < 16 * 36, "pruning is possible with the duplicates in place"
    pairs = wgp.pairs_float64(c, r2)
    for kind in graphref.RANKS:
        higher, lower = wg.rank_rule_witnesses(pairs, graphref.labels("own", n), graphref.rank_of(kind, n))
        assert higher > 0 and lower > 0, kind
    # 3 segments own two blocks each; of 7, six own one and the seventh is empty
    assert [len(pr.segment_blocks(n, s, 3)) for s in range(3)] == [2, 2, 2]
    assert [len(pr.segment_blocks(n, s, 7)) for s in range(7)] == [1, 1, 1, 1, 1, 1, 0]
    for n_seg in (1, 2, 3, 7):
        blocks = [b for s in range(n_seg) for b in pr.segment_blocks(n, s, n_seg)]
        assert sorted(blocks) == list(range(6))


def test_bounds_of_a_square_that_holds_no_pair():
    c, r, r2 = xg.stretched_case(700, 257)
    perm = pr.cell_order(c)
    for none in (float("nan"), 0.0, -0.0, -1.0, -float("inf")):
        assert xg.tile_bounds_r2(c, perm, none) == (0, 0)
    assert xg.tile_bounds_r2(c, perm, float("inf")) == (16 * 36, 16 * 36)
    assert xg.tile_bounds_r2(c, perm, r2, 6, 7) == (0, 0)


def test_the_block_rows_formula():
    assert xg.block_rows(300, 2) == 256 + 32 and xg.block_rows(1, 8) == 128 + 32 and xg.block_rows(1500, 5) == 3 * 128 + 32
    assert xg.block_rows(129, 2) == 128 + 32 and xg.block_rows(700, 8) == 128 + 32 and xg.block_rows(0, 3) == 0
    assert xg.block_rows(1500, 1) == 1536 + 32


@pytest.mark.parametrize("flaw", xg.FLAWS)
def test_the_flaws_keep_the_other_rows_pairs(probe, flaw):
    c, r, r2 = xg.stretched_case(300, 300)
    bad = xg.flawed(c, flaw)
    row = {"nan cell": 131, "inf cell": 40, "1e20 row": 200}[flaw]
    clean = graphref.brute_pairs(probe, c, r2)
    want = graphref.brute_pairs(probe, bad, r2)
    assert len(want) > 0 and not (want == row).any(), "the flawed row has no partner"
    assert np.array_equal(want, clean[~(clean == row).any(axis=1)])


def test_the_duplicate_tie_sits_on_the_boundary_of_blocks_0_and_1(oracle):
    import widesessionref as W
    c, fe, (a, p, m) = xg.duplicate_tie_case()
    assert c.shape == (384, 300)
    pos = {int(r): k for k, r in enumerate(pr.cell_order(c))}
    assert (pos[p], pos[m]) == (xg.BLOCK - 1, xg.BLOCK) and pos[a] // xg.BLOCK == 1 and p < m
    assert [pos[r] // xg.BLOCK % xg.DUPLICATE_SEGMENTS for r in (p, m)] == [0, 1], "blocks of different segments"
    assert (c[p] == c[m]).all() and fe[p] == fe[m] < fe[a] and W.d2_of(c, a, p) == 9.0 == W.d2_of(c, a, m)
    others = np.delete(np.arange(len(c)), [a, p, m])
    assert ((c[others].astype(np.float64) - c[a].astype(np.float64)) ** 2).sum(axis=1).min() > 9.0
    want = oracle.nearest_neighbors(c, fe)
    assert int(want[0][a]) == p and int(want[2][a]) == p and int(want[0][p]) == m and int(want[0][m]) == p


def test_the_block_shapes_cover_every_position_once_inside_the_payload():
    import widesessionref as W
    for n in xg.BLOCK_ROWS:
        for G in xg.BLOCK_SEGMENTS:
            assert xg.block_rows(n, G) == W.block_rows(n, G)
            seen = np.concatenate([W.segment_positions(n, g, G) for g in range(G)])
            assert sorted(seen.tolist()) == list(range(n))
            for g in range(G):
                loc = W.local_positions(n, g, G)
                assert len(loc) == 0 or loc.max() < xg.block_rows(n, G) - 32
                lo, hi = W.row_block(n, g, G)
                assert hi - lo <= xg.block_rows(n, G) - 32
    assert any(G > pr.n_blocks(n) for n in xg.BLOCK_ROWS for G in xg.BLOCK_SEGMENTS)


def test_the_flagged_block_cases_are_flagged():
    import widesessionref as W
    c, fe, want = xg.nan_cell_case(300)
    assert W.wide_flagged(c) and np.isnan(c[xg.FLAW]) and not np.isnan(fe).any()
    c, fe, want = xg.nan_fe_case(401)
    assert np.isnan(fe).any() and not W.wide_flagged(c)
    assert (want[2][np.isnan(fe)] == len(c) + 1).all(), "a NaN free energy has no lower neighbour"
