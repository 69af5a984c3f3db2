"""CPU: the premises of the pruned wide cross population sweep's GPU cases (tests/crosswidepruneref.py), with a numpy
joint-grid order whose cells come from the reference's row count: pruning is possible at every split shape and both
block-pair bounds are equal there; no such shape has a (query block, share) unit without a survivor, the edge case has
them beside units with one; the margin case puts each group into one block of its own set and their box gap is the
distance of the pair one ulp inside the radius; hand-made boxes; the block count of a gathered query range; and the
exact-path cap's premise at 1 500 x 1 500."""
import numpy as np
import pytest

import crosswidepruneref as ref
import widepruneref as wp

F32 = np.float32


@pytest.mark.parametrize("shape", sorted(ref.SPLIT_TABLE))
def test_split_blobs_can_be_pruned_and_both_bounds_are_equal(shape):
    n_q, n_r, d = shape
    Q, R = ref.split_sets(n_q, n_r, d)
    assert Q.shape == (n_q, d) and R.shape == (n_r, d)
    perm_q, perm_r = ref.joint_order(Q, R)
    assert sorted(perm_q.tolist()) == list(range(n_q)) and sorted(perm_r.tolist()) == list(range(n_r))
    r2max = ref.launch_r2max(ref.radii_for(d, 3))
    assert len(r2max) == 1
    g = ref.gaps(Q, R, perm_q, perm_r)
    assert g.shape == (ref.n_blocks(n_q), ref.n_blocks(n_r))
    lo, hi = ref.pair_bounds(g, r2max[0])
    assert (lo, g.size) == ref.SPLIT_TABLE[shape]
    assert lo == hi, "no block pair between the radius and the margin: the counter is pinned"
    assert hi < g.size, "pruning is possible"
    assert ref.tile_bounds(Q, R, perm_q, perm_r, ref.radii_for(d, 3)) == (16 * lo, 16 * hi)
    empty, units = ref.empty_units(g, r2max[0])
    assert empty == 0 and units == g.shape[0] * ref.shares(g.shape[1]), "every unit has a survivor"


def test_the_table_is_the_issue_s():
    assert ref.SPLIT_TABLE == {(300, 1500, 100): (22, 36), (1500, 1500, 65): (64, 144), (1500, 1500, 100): (64, 144),
                               (1500, 1500, 256): (64, 144), (700, 2100, 100): (49, 102), (1100, 8320, 80): (243, 585)}
    assert ref.shares(12) == 1 and ref.shares(17) == 2 and ref.shares(65) == 8


def test_queries_from_one_edge_leave_units_without_a_survivor_beside_units_with_one():
    Q, R = ref.mixed_units_sets()
    assert Q.shape == (1100, 80) and R.shape == (8320, 80)
    assert Q[:, 0].max() <= R[:, 0].min(), "the queries are the rows of lowest column 0"
    perm_q, perm_r = ref.joint_order(Q, R)
    g = ref.gaps(Q, R, perm_q, perm_r)
    r2max = ref.launch_r2max([ref.MIXED_RADIUS])
    assert r2max == [float(F32(1e-3) * F32(1e-3))]
    assert ref.pair_bounds(g, r2max[0]) == (2, 2) and g.size == 585
    assert ref.empty_units(g, r2max[0]) == (70, 72)


def test_the_cell_comes_from_the_reference_s_row_count():
    # the same queries against a short and a long reference from the same blobs: the longer reference makes smaller cells,
    # so the queries -- ordered on the reference's grid -- fall into more of them
    c = ref.stretched(300 + 8320, 80)
    Q = np.ascontiguousarray(c[:300])
    spans = []
    for n_r in (700, 8320):
        R = np.ascontiguousarray(c[300:300 + n_r])
        perm_q, _ = ref.joint_order(Q, R)
        b = ref.block_boxes(Q, perm_q)
        spans.append(float(((b[:, 1] - b[:, 0]) * (b[:, 3] - b[:, 2])).sum()))
    assert spans[1] < spans[0], "finer cells: tighter query boxes"
    # and an order of Q alone (cells from Q's own count) is another order
    perm_q, _ = ref.joint_order(Q, np.ascontiguousarray(c[300:]))
    assert perm_q.tolist() != wp.cell_order(Q).tolist()


def test_bounds_on_hand_made_boxes():
    # two query boxes against three reference boxes, (lo0, hi0, lo1, hi1)
    bq = np.array([[0, 1, 0, 1], [2, 2, 5, 5]], dtype=np.float64)
    br = np.array([[0, 1, 0, 1], [2, 3, 0, 1], [6, 7, 0, 1]], dtype=np.float64)
    g = ref.box_gap2(bq, br)
    assert g.shape == (2, 3)
    assert g.tolist() == [[0, 1, 25], [1 + 16, 16, 16 + 16]]
    assert ref.pair_bounds(g, 0.0) == (0, 0), "r2 = 0: not even overlapping boxes"
    assert ref.pair_bounds(g, 1.0) == (1, 2), "strictly below r2: the overlap; below 1.001 r2: the pair at gap 1 as well"
    assert ref.pair_bounds(g, 16.0) == (2, 3) and ref.pair_bounds(g, 16.02) == (3, 3)
    assert ref.pair_bounds(g, float("inf")) == (6, 6)
    # a rectangle is not symmetric: the transposed problem has the transposed gaps
    assert (ref.box_gap2(br, bq) == g.T).all()


def test_a_gathered_range_has_blocks_of_its_own():
    assert ref.query_blocks(0, 300) == 3 and ref.query_blocks(0, 0) == 0 and ref.query_blocks(5, 5) == 0
    # [37, 171) touches two blocks of the array and [100, 300) three; gathered, each is two blocks
    assert ref.query_blocks(37, 171) == 2 and ref.query_blocks(100, 300) == 2
    assert ref.query_blocks(127, 129) == 1, "two rows on either side of a block seam of the array: one block of the order"
    assert ref.query_blocks(0, 128) == 1 and ref.query_blocks(0, 129) == 2 and ref.query_blocks(299, 300) == 1
    Q, R = ref.split_sets(300, 1500, 100)
    perm_q, perm_r = ref.joint_order(np.ascontiguousarray(Q[37:171]), R)
    g = ref.gaps(Q, R, perm_q + 37, perm_r)
    assert g.shape == (ref.query_blocks(37, 171), 12)
    lo, hi = ref.tile_bounds(Q, R, perm_q + 37, perm_r, ref.radii_for(100, 3))
    assert 0 < lo <= hi <= 16 * 2 * 12
    assert ref.tile_bounds(Q, R, perm_q[:0], perm_r, [1.0]) == (0, 0)


def test_margin_case_premises():
    Q, R, r, (a, b, c, d) = ref.margin_sets()
    assert Q.shape == R.shape == (128, 80) and r == 3.0
    assert (Q[:, 0] <= 0).all() and (R[:, 0] >= F32(3.0) - F32(2.0 ** -22)).all()
    rest = np.ones(80, dtype=bool)
    rest[:2] = False
    for row in (b, c, d):
        assert (R[row][rest] == Q[a][rest]).all()
    assert tuple(Q[a, :2]) == (0.0, 0.0) and tuple(R[b, :2]) == (3.0, 0.0) and tuple(R[c, :2]) == (3.0, F32(2.0 ** -10))
    perm_q, perm_r = ref.joint_order(Q, R)
    g = ref.gaps(Q, R, perm_q, perm_r)
    assert g.shape == (1, 1)
    x, y = Q.astype(np.float64), R.astype(np.float64)
    assert g[0, 0] == ((x[a] - y[d]) ** 2).sum(), "the box gap IS the distance of the pair one ulp inside the radius"
    r2 = F32(r) * F32(r)
    assert F32(g[0, 0]) == np.nextafter(r2, F32(0)) and ((x[a] - y[b]) ** 2).sum() == 9.0
    assert F32(((x[a] - y[c]) ** 2).sum()) == np.nextafter(r2, F32(10))
    assert ref.tile_bounds(Q, R, perm_q, perm_r, [r]) == (16, 16)
    eight, eleven = wp.edge_radii()
    assert ref.tile_bounds(Q, R, perm_q, perm_r, eight) == (16, 16) and ref.tile_bounds(Q, R, perm_q, perm_r, eleven) == (32, 32)


@pytest.mark.parametrize("n_cols", [65, 256])
def test_the_exact_path_cap_can_be_met(n_cols):
    """the premise of the GPU module's cap: of the pairs of the surviving block pairs, those within the matrix-core window's
    half-width of a radius -- one origin and one scale over Q and R together -- are at most 1 %"""
    Q, R = ref.split_sets(1500, 1500, n_cols)
    perm_q, perm_r = ref.joint_order(Q, R)
    undecided, pairs = ref.exact_band_pairs(n_cols, Q, R, perm_q, perm_r, ref.radii_for(n_cols, 3))
    print(f"D={n_cols}: {undecided} pairs in the window of a radius, {pairs} surviving block pairs = "
          f"{100.0 * undecided / (1024 * 16 * pairs):.4f} % of their pairs")
    assert pairs == 64 and 0 < undecided <= 0.01 * 1024 * 16 * pairs
