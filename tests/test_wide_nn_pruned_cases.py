"""CPU: the premises of the pruned wide neighbour sweep's GPU cases (tests/widennpruneref.py), with a numpy cell order:
pruning happens at every stretched shape and both counter bounds are equal there; what constant free energies and a
gradient do to ring 2; the cross-block tie and the margin cases are what they claim to be; and the ring rule itself
against long-double arithmetic (clustering_amd/bin/test_wide_nn_prune)."""
import os
import subprocess

import numpy as np
import pytest

import wideref
import widepruneref as pr
import widennpruneref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.mark.parametrize("shape", sorted(ref.STRETCHED_TABLE))
def test_pruning_happens_on_the_stretched_blobs_and_both_bounds_are_equal(shape):
    c, fe, _ = ref.stretched_case(*shape)
    perm = pr.cell_order(c)
    lo, hi, s1_lo, s1_hi = ref.pair_bounds(c, fe, perm)
    nb = pr.n_blocks(len(c))
    assert (lo, nb * nb) == ref.STRETCHED_TABLE[shape]
    assert lo == hi and s1_lo == s1_hi, "no block pair between a bound and its margin: the counter is pinned"
    assert hi < nb * nb, "pruning happens"
    assert s1_lo == pr.STRETCHED_TABLE[shape][0], "ring 1 at these free energies: the population sweep's pairs"
    assert ref.tile_bounds(c, fe, perm) == (16 * lo, 16 * hi)


def test_free_energies_decide_ring_2():
    c, fe, _ = ref.stretched_case(2100, 100)
    perm = pr.cell_order(c)
    const = ref.pair_bounds(c, np.zeros(len(c), dtype=np.float32), perm)
    assert const == (ref.CONSTANT_2100,) * 4, "no row lies lower than another: ring 2 is empty"
    assert ref.CONSTANT_2100 == pr.STRETCHED_TABLE[(2100, 100)][0]
    grad = ref.pair_bounds(c, np.ascontiguousarray(c[:, 0]), perm)
    assert grad == (ref.GRADIENT_2100, ref.GRADIENT_2100, ref.CONSTANT_2100, ref.CONSTANT_2100)
    # the block that holds the global minimum of the population free energies sweeps everything
    top = int(np.argmin(fe))
    qb = int(np.nonzero(perm == top)[0][0]) // ref.BLOCK
    _, _, _, lower, upper = ref.block_sets(c, fe, perm, qb)
    assert lower.all() and upper.all()


def test_three_blocks_are_all_seed_blocks():
    c, fe, _ = ref.stretched_case(300, 100)
    assert ref.pair_bounds(c, fe, pr.cell_order(c))[:2] == (9, 9)
    assert ref.seed_blocks(0, 3) == [0, 1] and ref.seed_blocks(1, 3) == [0, 1, 2] and ref.seed_blocks(2, 3) == [1, 2]
    assert ref.seed_blocks(0, 1) == [0] and ref.seed_blocks(64, 65) == [63, 64]


def test_segments_add_up():
    c, fe, _ = ref.stretched_case(2100, 100)
    perm = pr.cell_order(c)
    whole = ref.pair_bounds(c, fe, perm)
    for n_seg in (2, 3, 8):
        parts = [ref.pair_bounds(c, fe, perm, s, n_seg) for s in range(n_seg)]
        assert tuple(sum(p[k] for p in parts) for k in range(4)) == whole


def test_ties_on_the_stretched_layout_stay_ties():
    c, stars, dups = wideref.ties_case(300, 100)
    c = c.copy()
    c[:, :2] *= F32(4)
    x = c.astype(np.float64)
    for q, ring in stars:
        d2 = ((x[ring] - x[q]) ** 2).sum(axis=1)
        assert (d2 == d2[0]).all() and d2[0] == 16.0 * 2.0 ** -12
        others = np.ones(len(c), dtype=bool)
        others[[q] + list(ring)] = False
        assert ((x[others] - x[q]) ** 2).sum(axis=1).min() > d2[0]
    for copy, orig in dups:
        assert (c[copy] == c[orig]).all()


def test_cross_block_tie_premises(oracle):
    c, fe, (a, p, q) = ref.cross_block_tie_case()
    assert c.shape == (384, 100) and q < a < p
    perm = pr.cell_order(c)
    blocks = [set(perm[128 * b:128 * (b + 1)].tolist()) for b in range(3)]
    assert blocks[0] == set(range(2, 384, 3)) and blocks[1] == set(range(1, 384, 3)) and blocks[2] == set(range(0, 384, 3))
    assert p in blocks[0] and a in blocks[1] and q in blocks[2], "p comes FIRST in the order and has the HIGHER row index"
    x = c.astype(np.float64)
    d2 = ((x - x[a]) ** 2).sum(axis=1)
    assert d2[p] == 9.0 and d2[q] == 9.0
    rest = np.ones(len(c), dtype=bool)
    rest[[a, p, q]] = False
    assert d2[rest].min() > 9.0
    assert fe[p] == fe[q] < fe[a]
    nn = oracle.nearest_neighbors(c, fe)
    assert int(nn[0][a]) == q and int(nn[2][a]) == q, "the least (d2, ROW): q"
    assert nn[1][a] == 9.0 and nn[3][a] == 9.0
    pos = {int(r): k for k, r in enumerate(perm)}
    assert pos[p] < pos[q], "a merge on positions would answer p"


@pytest.mark.parametrize("which", [-1, 0, 1])
def test_margin_case_premises(oracle, which):
    c, fe, (a, a2), gap2 = ref.margin_case(which)
    assert c.shape == (384, 80)
    perm = pr.cell_order(c)
    groups = [sorted(np.concatenate([np.arange(g, 384, 6), np.arange(g + 1, 384, 6)]).tolist()) for g in (0, 2, 4)]
    for b in range(3):
        assert sorted(perm[128 * b:128 * (b + 1)].tolist()) == groups[b], "each group fills one block"
    boxes = pr.block_boxes(c, perm)
    g = pr.box_gap2(boxes, boxes)
    far2 = ref.MARGIN_FAR2
    assert far2 == F32(1.0001) * F32(9.0) and F32(g[0, 2]) == F32(gap2)
    want = {-1: np.nextafter(far2, F32(0)), 0: far2, 1: np.nextafter(far2, F32(100))}[which]
    assert F32(gap2) == want, "one ulp inside, on, one ulp outside far2_nn"
    # the float gap the device forms: two differences, two squares, one sum
    dx, dy = F32(boxes[2, 0]) - F32(boxes[0, 1]), F32(boxes[2, 2]) - F32(boxes[0, 3])
    assert F32(F32(dx * dx) + F32(dy * dy)) == want
    # the bound of block 0 after its seed blocks 0 and 1 is d2(a, a2) = 9: a pair inside the query block
    nn = oracle.nearest_neighbors(c, fe)
    in_a = np.array(groups[0])
    assert int(nn[0][a]) == a2 and nn[1][a] == 9.0 and float(nn[1][in_a].max()) == 9.0
    rest = in_a[(in_a != a) & (in_a != a2)]
    assert (nn[1][rest] == 0.0).all() and (nn[1][np.array(groups[1] + groups[2])] == 0.0).all(), "duplicates elsewhere"
    assert (nn[2] == len(c) + 1).all(), "constant free energies: no hd anywhere, ring 2 is empty"
    # float64 bounds: the block pair lies between f_lo B and f_hi B in all three cases
    assert ref.pair_bounds(c, fe, perm)[:2] == (7, 8)


def test_the_ring_rule_against_long_double_arithmetic():
    exe = os.path.join(ROOT, "clustering_amd", "bin", "test_wide_nn_prune")
    assert os.path.exists(exe), "build() makes clustering_amd/bin/test_wide_nn_prune"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
    assert int(out.stdout.split()[1]) > 100000
