"""CPU: the case generators of the wide radius-graph tests (tests/widegraphref.py) hold what the GPU module
(tests/test_gpu_wide_graph.py) relies on: every case has pairs; the boundary case has pairs on the radius and one ulp to
either side of it; the sparse case has pairs whose two ends lie in different reference shares and different query
blocks, and stays sparse; the min-edge cases have tied partners and exercise both branches of the smallest-rank rule."""
import numpy as np
import pytest

import graphref
import wideref
import widegraphref as wg

F32 = np.float32


@pytest.mark.parametrize("n_cols", wg.COLS)
def test_every_column_case_has_pairs(probe, n_cols):
    c, r, r2 = wg.blob_case(200, n_cols)
    pairs = graphref.brute_pairs(probe, c, r2)
    assert 0 < len(pairs) < 200 * 199 // 2


@pytest.mark.parametrize("n_rows", [n for n in wg.ROWS if n >= 33])
def test_every_row_case_has_pairs(probe, n_rows):
    c, r, r2 = wg.blob_case(n_rows, 100)
    assert len(graphref.brute_pairs(probe, c, r2)) > 0
    assert wg.shares_of(1500) == 1 and wg.shares_of(2100) == 2 and wg.shares_of(4100) == 4


def test_boundary_case_has_pairs_on_and_one_ulp_to_either_side_of_the_radius(probe):
    c, r, groups = wideref.boundary_case(300, 80)
    r2 = wg.square(r)
    assert r2 == F32(9.0)
    d2 = probe.pairwise_d2(c)
    keys = set(graphref.keys(graphref.brute_pairs(probe, c, r2), len(c)).tolist())
    for a, b, cc, d in groups:
        assert d2[a, b] == r2 and d2[a, cc] == np.nextafter(r2, F32(np.inf)) and d2[a, d] == np.nextafter(r2, F32(0))
        assert int(graphref.keys([[a, d]], len(c))[0]) in keys
        assert int(graphref.keys([[a, b]], len(c))[0]) not in keys and int(graphref.keys([[a, cc]], len(c))[0]) not in keys


def test_sparse_case_splits_pairs_over_shares_and_blocks(probe):
    c, r, r2 = wg.sparse_case()
    n = len(c)
    assert c.shape == wg.SPARSE_SHAPE and wg.shares_of(n) == 4
    pairs = graphref.brute_pairs(probe, c, r2)
    assert 500 < len(pairs) < 20 * n, "a list that stays sparse"
    split = wg.split_pairs(pairs, n)
    assert len(split) > 100
    # ... from every share to every other share
    s = (split // wg.BLOCK_ROWS) % 4
    assert len({(int(a), int(b)) for a, b in s}) == 12


@pytest.mark.parametrize("n_rows,n_cols", [(300, 100), (200, 256)])
def test_min_edge_cases_have_ties_and_both_branches_of_the_rank_rule(probe, n_rows, n_cols):
    c, stars, dups = wideref.ties_case(n_rows, n_cols)
    r2 = wg.square(wg.blob_radius(n_cols))
    d2 = probe.pairwise_d2(c)
    pairs = graphref.pairs_of(d2, r2)
    assert len(pairs) > 0
    for q, ring in stars:
        assert len({float(d2[q, x]) for x in ring}) == 1 and d2[q, ring[0]] < r2, "partners that tie in d2"
    for copy, orig in dups:
        assert d2[copy, orig] == 0 and (d2[copy] == d2[orig]).all(), "a duplicated row: every partner ties"
    for lab in ("own", "any"):
        comp = graphref.labels(lab, n_rows)
        for kind in graphref.RANKS:
            higher, lower = wg.rank_rule_witnesses(pairs, comp, graphref.rank_of(kind, n_rows))
            assert higher > 0 and lower > 0, (lab, kind, higher, lower)
        assert (graphref.min_edge_brute(pairs, comp, graphref.rank_of("random", n_rows), n_rows) != graphref.ALL_ONES).any()
    assert (graphref.min_edge_brute(pairs, graphref.labels("one", n_rows), graphref.rank_of("random", n_rows), n_rows)
            == graphref.ALL_ONES).all(), "one component: no pair leaves it"


def test_forest_shapes(probe):
    c, r2 = wg.chain_case(150, 65)
    pairs = graphref.brute_pairs(probe, c, r2)
    assert np.array_equal(pairs, np.stack([np.arange(149), np.arange(1, 150)], axis=1))
    c, r2, side, (p, q), (d, _) = graphref.bridge(100)
    pairs = graphref.brute_pairs(probe, c, r2)
    crossing = pairs[side[pairs[:, 0]] != side[pairs[:, 1]]]
    assert len(crossing) == 1 and set(crossing[0].tolist()) == {p, q}
    assert len(np.unique(graphref.components(len(c), pairs))) == 1
    c, r, r2 = wg.blob_case(200, 100)
    assert len(graphref.brute_pairs(probe, c, 1.0e6)) == 200 * 199 // 2
    assert len(graphref.brute_pairs(probe, c, 1.0e-6)) == 0


@pytest.mark.parametrize("n_cols", [65, 256])
def test_the_exact_path_case_is_the_population_tests_window(n_cols):
    """the cap of the GPU module is held at the window of one threshold, the one the population tests use: the share of
    pairs within 2 eps of it stays under 1 %"""
    c, r, r2 = wg.blob_case(1500, n_cols)
    x = c.astype(np.float64)
    g = (x * x).sum(axis=1)
    d2 = np.maximum(g[:, None] + g[None, :] - 2.0 * (x @ x.T), 0.0)
    off = d2[~np.eye(len(c), dtype=bool)]
    e = wideref.eps(n_cols, c, float(r2))
    share = float((np.abs(off - float(r2)) < 2.0 * e).mean())
    print(f"D={n_cols}: r2={float(r2):.4f} eps={e:.3e} share within 2 eps = {100 * share:.4f} %")
    assert e > 0 and share < 0.01
