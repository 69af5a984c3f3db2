"""CPU: the premises of the pruned wide radius graph's GPU cases (tests/widegraphpruneref.py), with a numpy cell order:
every stretched shape has a dropped and a surviving block pair at the radius the table was made for, the order is not the
identity and holds pairs whose rows stand the other way round in it, the small radius leaves (query block, share) units
without a survivor, and the boundary pairs are met across two blocks where the cases say so."""
import numpy as np
import pytest

import graphref
import widegraphpruneref as wgp
import widegraphref as wg
import widepruneref as ref
import wideref

F32 = np.float32


@pytest.mark.parametrize("shape", wgp.STRETCHED)
def test_every_stretched_shape_has_a_dropped_and_a_surviving_block_pair(shape):
    n, d = shape
    c, r, r2 = wgp.stretched_case(n, d)
    assert r == max(ref.radii_for(d, 3)) and r2 == F32(F32(r) * F32(r)), "the radius the table was made for"
    assert [float(r2)] == ref.launch_r2max(ref.radii_for(d, 3)) == ref.launch_r2max([r])
    perm = ref.cell_order(c)
    assert not np.array_equal(perm, np.arange(n)), "the order is not the identity"
    nb = ref.n_blocks(n)
    lo, hi = ref.pair_bounds(ref.block_boxes(c, perm), float(r2))
    assert (lo, nb * nb) == ref.STRETCHED_TABLE[shape] and lo == hi
    assert nb <= lo < nb * nb, "every block meets itself, and some block pair is dropped"
    assert wgp.tile_bounds_r2(c, perm, r2) == ref.tile_bounds(c, perm, [r]) == (16 * lo, 16 * hi)
    assert 16 * lo < 16 * nb * nb, "the lower bound of the counter lies strictly below all tile pairs"


def test_block_counts_and_shares_of_the_shapes():
    assert [ref.n_blocks(n) for n, _ in wgp.STRETCHED] == [6, 12, 17, 65]
    assert [ref.shares(ref.n_blocks(n)) for n, _ in wgp.STRETCHED] == [1, 1, 2, 8]


@pytest.mark.parametrize("shape", [(700, 100), (1500, 100), (2100, 100)])
def test_pairs_stand_the_other_way_round_in_the_order(shape):
    # (a blob that falls into one cell keeps its rows in row order -- the sort is stable -- so 700 rows have a handful of
    #  such pairs, 1 500 and 2 100 rows, whose blobs spread over several cells, thousands)
    c, r, r2 = wgp.stretched_case(*shape)
    perm = ref.cell_order(c)
    pairs = wgp.pairs_float64(c, r2)
    assert len(pairs) > 1000 and (pairs[:, 0] < pairs[:, 1]).all()
    turned = wgp.pairs_against_the_order(pairs, perm)
    inv = wgp.inverse(perm)
    assert 0 < len(turned) < len(pairs) - 100, "pairs of either kind"
    assert (inv[turned[:, 1]] < inv[turned[:, 0]]).all() and (turned[:, 0] < turned[:, 1]).all()
    if shape[0] == 700:
        return
    # ... many of them inside one block (decided under the diagonal rule), many across two blocks
    same = inv[turned[:, 0]] // wgp.BLOCK == inv[turned[:, 1]] // wgp.BLOCK
    assert same.sum() > 100 and (~same).sum() > 1000


def test_the_small_radius_holds_the_duplicates_only_and_leaves_units_without_a_survivor():
    c, r, r2, dups = wgp.small_radius_case()
    assert len(dups) == 24 and len(np.unique(dups)) == 48 and (c[dups[:, 0]] == c[dups[:, 1]]).all()
    perm = ref.cell_order(c)
    empty, units = ref.empty_units(c, perm, float(r2))
    assert units == 8 * 65 and empty > 0
    # nothing but the duplicates within 1e-3: the nearest other pair of this data is far beyond it
    x = c.astype(np.float64)
    sample = x[::13]
    d2 = ((sample[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    assert (np.sort(d2, axis=1)[:, 2] > 0.1).all()
    blocks = np.array([wgp.blocks_of(pair, perm) for pair in dups])
    # (a cell holds several blocks, in row order: a duplicate and its original meet across blocks whose boxes overlap)
    assert (blocks[:, 0] != blocks[:, 1]).sum() >= 10 and (blocks[:, 0] == blocks[:, 1]).any()


def test_the_min_edge_case_has_tied_partners_and_both_rank_branches():
    c, r, r2, dups = wgp.min_edge_case()
    assert c.shape == wgp.MIN_EDGE_SHAPE and (c[dups[:, 0]] == c[dups[:, 1]]).all()
    perm = ref.cell_order(c)
    lo, hi = ref.pair_bounds(ref.block_boxes(c, perm), float(r2))
    assert 6 <= lo == hi < 36, "pruning is possible with the duplicates in place"
    pairs = wgp.pairs_float64(c, r2)
    n = len(c)
    for kind in graphref.RANKS:
        higher, lower = wg.rank_rule_witnesses(pairs, graphref.labels("own", n), graphref.rank_of(kind, n))
        assert higher > 0 and lower > 0, kind
    # 3 and 7 segments over 6 blocks: every block in exactly one segment, the seventh segment without a block
    for n_seg in (3, 7):
        blocks = [list(ref.segment_blocks(n, s, n_seg)) for s in range(n_seg)]
        assert sorted(b for bl in blocks for b in bl) == list(range(6))
    assert list(ref.segment_blocks(n, 6, 7)) == []


def test_the_boundary_pairs_lie_in_different_blocks_where_the_cases_say_so():
    c, r, groups = wideref.boundary_case(*wgp.BOUNDARY_SHAPE)
    perm = ref.cell_order(c)
    assert ref.n_blocks(len(c)) == 3
    for g, rows in enumerate(groups):
        a, b, cc, d = wgp.blocks_of(rows, perm)
        assert (a not in (b, cc, d)) == (g in wgp.BOUNDARY_SPLIT_GROUPS), (g, rows)
    a, b, cc, d = wgp.blocks_of(groups[2], perm)
    assert a == b == d, "the last group: the pair on the radius and the pair inside it within one block"
    lo, hi = wgp.tile_bounds_r2(c, perm, wg.square(r))
    assert lo == hi == 16 * 9, "blobs of sigma 0.3 at r = 3: nothing to prune"
    c, r, rows = ref.margin_case()
    assert wgp.blocks_of(rows, ref.cell_order(c)) == [0, 1, 1, 1]
    assert wgp.tile_bounds_r2(c, ref.cell_order(c), wg.square(r)) == (64, 64)


def test_bounds_of_a_square_that_holds_no_pair():
    c, r, r2 = wgp.stretched_case(700, 100)
    perm = ref.cell_order(c)
    for none in (float("nan"), 0.0, -0.0, -1.0, -float("inf")):
        assert wgp.tile_bounds_r2(c, perm, none) == (0, 0)
    assert wgp.tile_bounds_r2(c, perm, float("inf")) == (16 * 36, 16 * 36)
    assert wgp.tile_bounds_r2(c, perm, r2, 6, 7) == (0, 0)
    parts = [wgp.tile_bounds_r2(c, perm, r2, s, 3) for s in range(3)]
    assert tuple(map(sum, zip(*parts))) == wgp.tile_bounds_r2(c, perm, r2)
