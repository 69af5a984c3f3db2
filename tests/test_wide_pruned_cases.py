"""CPU: the premises of the pruned wide population sweep's GPU cases (tests/widepruneref.py), with a numpy cell order:
pruning is possible at every stretched shape and both block-pair bounds are equal there; the bounds function on
hand-made boxes; the two groups of the margin case fill one block each and their box gap is the distance of the pair
one ulp inside the radius; and the survivor rule itself against long-double arithmetic (clustering_amd/bin/test_wide_prune)."""
import os
import subprocess

import numpy as np
import pytest

import widepruneref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.mark.parametrize("shape", sorted(ref.STRETCHED_TABLE))
def test_stretched_blobs_can_be_pruned_and_both_bounds_are_equal(shape):
    n, d = shape
    c = ref.stretched(n, d)
    perm = ref.cell_order(c)
    assert sorted(perm.tolist()) == list(range(n))
    r2max = ref.launch_r2max(ref.radii_for(d, 3))
    assert len(r2max) == 1
    lo, hi = ref.pair_bounds(ref.block_boxes(c, perm), r2max[0])
    assert (lo, ref.n_blocks(n) ** 2) == ref.STRETCHED_TABLE[shape]
    assert lo == hi, "no block pair between the radius and the margin: the counter is pinned"
    assert hi < ref.n_blocks(n) ** 2, "pruning is possible"
    assert ref.tile_bounds(c, perm, ref.radii_for(d, 3)) == (16 * lo, 16 * hi)


def test_the_radii_lie_around_the_intra_blob_distance():
    for d in (65, 100, 256):
        c = ref.stretched(400, d).astype(np.float64)
        lab = np.round((c[:, 0] / 4 + 1)).astype(int)
        same = c[lab == 0]
        d2 = ((same[:, None, :] - same[None, :, :]) ** 2).sum(-1)
        med = np.sqrt(np.median(d2[np.triu_indices(len(same), 1)]))
        r = ref.radii_for(d, 8)
        assert min(r) < med < max(r) and r != sorted(r)


def test_bounds_on_hand_made_boxes():
    # three unit boxes in a row, 1 apart and 3 apart; a point; boxes are (lo0, hi0, lo1, hi1)
    boxes = np.array([[0, 1, 0, 1], [2, 3, 0, 1], [6, 7, 0, 1], [2, 2, 5, 5]], dtype=np.float64)
    g = ref.box_gap2(boxes, boxes)
    assert (np.diag(g) == 0).all() and (g == g.T).all()
    assert g[0, 1] == 1 and g[1, 2] == 9 and g[0, 2] == 25 and g[1, 3] == 16 and g[0, 3] == 1 + 16
    assert ref.pair_bounds(boxes, 0.0) == (0, 0), "r2 = 0: not even a block with itself"
    assert ref.pair_bounds(boxes, 1.0) == (4, 6), "strictly below r2: the diagonal; below 1.001 r2: the pair at gap 1 as well"
    assert ref.pair_bounds(boxes, 1.0005) == (6, 6)
    assert ref.pair_bounds(boxes, 9.0) == (6, 8)
    assert ref.pair_bounds(boxes, float("inf")) == (16, 16)
    assert ref.pair_bounds(boxes, 9.5, query_blocks=[1]) == (3, 3) and ref.pair_bounds(boxes, 9.5, query_blocks=[]) == (0, 0)
    # touching and overlapping boxes: gap 0
    t = np.array([[0, 1, 0, 1], [1, 2, 1, 2], [0.5, 1.5, 0.5, 1.5]], dtype=np.float64)
    assert (ref.box_gap2(t, t) == 0).all()


def test_launch_maxima_and_segment_blocks():
    assert ref.launch_r2max([1.0, 3.0, 2.0]) == [9.0]
    assert ref.launch_r2max([0.5] * 8 + [2.0]) == [0.25, 4.0]
    assert ref.launch_r2max([1e30]) == [float("inf")] and ref.launch_r2max([float("nan"), 0.0]) == [0.0]
    eight, eleven = ref.edge_radii()
    assert len(eight) == 8 and len(eleven) == 11 and ref.launch_r2max(eleven)[0] == float("inf")
    assert list(ref.segment_blocks(1500, 0, 0)) == list(range(12))
    assert list(ref.segment_blocks(1500, 1, 5)) == [1, 6, 11] and list(ref.segment_blocks(1500, 12, 40)) == []
    assert sorted(b for s in range(5) for b in ref.segment_blocks(1500, s, 5)) == list(range(12))


def test_the_small_radii_leave_units_without_a_survivor():
    c = ref.stretched(8320, 80)
    perm = ref.cell_order(c)
    r2max = ref.launch_r2max([1e-3, 0.0])
    assert r2max == [float(F32(1e-3) * F32(1e-3))]
    assert ref.shares(65) == 8 and ref.shares(12) == 1 and ref.shares(17) == 2 and ref.shares(3000) == 64
    empty, units = ref.empty_units(c, perm, r2max[0])
    assert units == 8 * 65 and empty == 71, "(query block, share) units no block of which comes near the query block"
    lo, hi = ref.pair_bounds(ref.block_boxes(c, perm), r2max[0])
    assert 65 <= lo == hi == 657 < 65 * 65, "every block meets itself; the blocks of a blob overlap in the plane"


def test_margin_case_premises():
    c, r, (a, b, cc, d) = ref.margin_case()
    assert c.shape == (256, 80) and r == 3.0
    perm = ref.cell_order(c)
    assert sorted(perm[:128].tolist()) == list(range(0, 256, 2)), "group A fills block 0"
    assert sorted(perm[128:].tolist()) == list(range(1, 256, 2)), "group B fills block 1"
    assert (c[0::2, 0] <= 0).all() and (c[1::2, 0] >= F32(3.0) - F32(2.0 ** -22)).all()
    rest = np.ones(80, dtype=bool)
    rest[:2] = False
    for row in (b, cc, d):
        assert (c[row][rest] == c[a][rest]).all()
    assert tuple(c[a, :2]) == (0.0, 0.0) and tuple(c[b, :2]) == (3.0, 0.0) and tuple(c[cc, :2]) == (3.0, F32(2.0 ** -10))
    boxes = ref.block_boxes(c, perm)
    gap2 = ref.box_gap2(boxes, boxes)[0, 1]
    x = c.astype(np.float64)
    assert gap2 == ((x[a] - x[d]) ** 2).sum(), "the box gap IS the distance of the pair one ulp inside the radius"
    r2 = F32(r) * F32(r)
    assert F32(gap2) == np.nextafter(r2, F32(0)) and ((x[a] - x[b]) ** 2).sum() == 9.0
    assert F32(((x[a] - x[cc]) ** 2).sum()) == np.nextafter(r2, F32(10))
    assert ref.tile_bounds(c, perm, [r]) == (64, 64)
    eight, eleven = ref.edge_radii()
    assert ref.tile_bounds(c, perm, eight) == (64, 64) and ref.tile_bounds(c, perm, eleven) == (128, 128)


def test_the_survivor_rule_against_long_double_arithmetic():
    exe = os.path.join(ROOT, "clustering_amd", "bin", "test_wide_prune")
    assert os.path.exists(exe), "build() makes clustering_amd/bin/test_wide_prune"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
    assert int(out.stdout.split()[1]) > 100000
