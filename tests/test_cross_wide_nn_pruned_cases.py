"""CPU: the premises of the pruned wide cross neighbour sweep's GPU cases (tests/crosswidennpruneref.py), with the numpy
joint-grid order: the seed of every query block is unambiguous at every case, pruning happens at every split shape and both
counter bounds are equal there; what the free energies do to ring 2; the cross-block tie, the margin cases and the far
queries are what they claim to be; and the seed rule itself against long-double arithmetic
(clustering_amd/bin/test_wide_cross_seed)."""
import os
import subprocess

import numpy as np
import pytest

import crossref
import crosswidepruneref as cp
import crosswidennpruneref as ref
import widepruneref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def d2_64(Q, R):
    q, r = Q.astype(np.float64), R.astype(np.float64)
    return ((q[:, None, :] - r[None, :, :]) ** 2).sum(axis=2)


@pytest.mark.parametrize("shape", sorted(ref.SPLIT_TABLE))
def test_pruning_happens_on_the_split_sets_and_both_bounds_are_equal(shape):
    Q, R, fe_q, fe_r = ref.split_case(*shape)
    perm_q, perm_r = cp.joint_order(Q, R)
    lo, hi, s1_lo, s1_hi = ref.pair_bounds(Q, R, fe_q, fe_r, perm_q, perm_r)   # (asserts the seed premise)
    all_pairs = pr.n_blocks(len(Q)) * pr.n_blocks(len(R))
    assert (lo, all_pairs) == ref.SPLIT_TABLE[shape]
    assert lo == hi and s1_lo == s1_hi, "no block pair between a bound and its margin: the counter is pinned"
    assert hi < all_pairs, "pruning happens"
    assert s1_lo >= pr.n_blocks(len(Q)), "a seed block pair per query block at least"
    assert ref.tile_bounds(Q, R, fe_q, fe_r, perm_q, perm_r) == (16 * lo, 16 * hi)
    # nn only: no ring 2
    assert ref.pair_bounds(Q, R, None, None, perm_q, perm_r) == (s1_lo, s1_hi, s1_lo, s1_hi)
    counts, bounds = ref.block_counts(Q, R, fe_q, fe_r, perm_q, perm_r)
    assert np.isfinite(bounds[:, 0]).all(), "the seed block has a row and nothing is excluded: B_nn is finite"


@pytest.mark.parametrize("shape", [(1, 300, 100), (300, 1, 100), (33, 129, 100), (129, 33, 100), (1500, 300, 100)])
def test_the_seed_is_unambiguous_at_the_small_rectangles(shape):
    Q, R, fe_q, fe_r = ref.split_case(*shape)
    perm_q, perm_r = cp.joint_order(Q, R)
    lo, hi, _, _ = ref.pair_bounds(Q, R, fe_q, fe_r, perm_q, perm_r)
    assert pr.n_blocks(len(Q)) <= lo <= hi <= pr.n_blocks(len(Q)) * pr.n_blocks(len(R))


def test_free_energies_decide_ring_2():
    Q, R, fe_q, fe_r = ref.split_case(700, 2100, 100)
    perm_q, perm_r = cp.joint_order(Q, R)
    nn_only = ref.pair_bounds(Q, R, None, None, perm_q, perm_r)
    zq, zr = np.zeros(len(Q), dtype=np.float32), np.zeros(len(R), dtype=np.float32)
    # the largest free energy of every query block AT the reference's least, and below it: ring 2 is empty
    assert ref.pair_bounds(Q, R, zq, zr, perm_q, perm_r) == nn_only
    assert ref.pair_bounds(Q, R, zq - F32(1.0), zr, perm_q, perm_r) == nn_only
    # a gradient shifted by half a blob distance: no query has a lower reference in its own blob, B_hd = +inf, and its
    # block meets every block that holds a lower row -- and only those
    gq, gr = ref.shifted_gradient(Q, R)
    counts, bounds = ref.block_counts(Q, R, gq, gr, perm_q, perm_r)
    open_blocks = np.flatnonzero(np.isinf(bounds[:, 1]))
    assert len(open_blocks) > 0, "a query without a lower reference after ring 1"
    assert (crossref.expect_nn(d2_64(Q, R).astype(np.float32), gq, gr)[2] == len(R) + 1).any()
    fe_min, fe_max = ref.fe_ends(gq, gr, perm_q, perm_r)
    for qb in open_blocks:
        _, s1_lo, s1_hi, lower, upper, _, _ = ref.block_sets(Q, R, gq, gr, perm_q, perm_r, int(qb))
        assert (lower == (s1_lo | (fe_min < fe_max[qb]))).all() and (upper == (s1_hi | (fe_min < fe_max[qb]))).all()
    assert counts[:, 0].sum() > nn_only[0], "ring 2 adds block pairs"


def test_cross_block_tie_premises():
    Q, R, fe_q, fe_r, (a_q, p, q) = ref.cross_block_tie_sets()
    assert Q.shape == (128, 100) and R.shape == (384, 100) and q < p
    perm_q, perm_r = cp.joint_order(Q, R)
    blocks = [set(perm_r[128 * b:128 * (b + 1)].tolist()) for b in range(3)]
    assert p in blocks[0] and q in blocks[2], "p comes FIRST in the reference's order and has the HIGHER row index"
    d2 = d2_64(Q[a_q:a_q + 1], R)[0]
    assert d2[p] == 9.0 and d2[q] == 9.0
    rest = np.ones(len(R), dtype=bool)
    rest[[p, q]] = False
    assert d2[rest].min() > 9.0
    assert fe_r[p] == fe_r[q] < fe_q[a_q]
    want = crossref.expect_nn(d2_64(Q, R).astype(np.float32), fe_q, fe_r)
    assert int(want[0][a_q]) == q and int(want[2][a_q]) == q and want[1][a_q] == 9.0 and want[3][a_q] == 9.0
    ref.seed_premise(pr.block_boxes(Q, perm_q), pr.block_boxes(R, perm_r))


@pytest.mark.parametrize("which", [-1, 0, 1])
def test_margin_sets_premises(which):
    Q, R, fe_q, fe_r, a_q, gap2 = ref.margin_sets(which)
    assert Q.shape == (128, 80) and R.shape == (384, 80)
    perm_q, perm_r = cp.joint_order(Q, R)
    # the reference's order: the copy of A (rows 3k), M (3k + 1), B (3k + 2), one block each
    for b in range(3):
        assert sorted(perm_r[128 * b:128 * (b + 1)].tolist()) == list(range(b, 384, 3)), "each group fills one block"
    bq, br = pr.block_boxes(Q, perm_q), pr.block_boxes(R, perm_r)
    assert (ref.seed_premise(bq, br) == [0]).all(), "the seed of the query block is the copy of A"
    far2 = ref.MARGIN_FAR2
    want = {-1: np.nextafter(far2, F32(0)), 0: far2, 1: np.nextafter(far2, F32(100))}[which]
    assert F32(gap2) == want, "one ulp inside, on, one ulp outside far2_nn"
    # the float gap the device forms: two differences, two squares, one sum
    dx, dy = F32(br[2, 0]) - F32(bq[0, 1]), F32(br[2, 2]) - F32(bq[0, 3])
    assert F32(F32(dx * dx) + F32(dy * dy)) == want
    g = pr.box_gap2(bq, br)[0]
    assert g[0] == 0.0 and 1.0 < g[1] < 2.0, "the copy of A overlaps the queries, M lies inside the bound"
    # the bound after the seed launch is d2(a, a2) = 9 exactly: every other query has an exact copy in the seed block
    d2 = d2_64(Q, R[0::3])
    nn = d2.min(axis=1)
    assert nn[a_q] == 9.0 and (np.delete(nn, a_q) == 0.0).all()
    assert d2_64(Q[a_q:a_q + 1], R).min() == 9.0, "no reference of M or B is nearer to a"
    # float64 bounds: the far block lies between F_LO B and F_HI B in all three cases
    assert ref.pair_bounds(Q, R, fe_q, fe_r, perm_q, perm_r)[:2] == (2, 3)


def test_far_queries_still_have_a_seed_and_a_finite_bound():
    Q, R, fe_q, fe_r = ref.far_sets()
    perm_q, perm_r = cp.joint_order(Q, R)
    g = cp.gaps(Q, R, perm_q, perm_r)
    assert g.min() > 5000.0, "every box of the reference is far from every box of the queries"
    counts, bounds = ref.block_counts(Q, R, fe_q, fe_r, perm_q, perm_r)
    assert np.isfinite(bounds[:, 0]).all() and (counts[:, 2] >= 1).all()


def test_the_seed_rule_against_long_double_arithmetic():
    exe = os.path.join(ROOT, "clustering_amd", "bin", "test_wide_cross_seed")
    assert os.path.exists(exe), "build() makes clustering_amd/bin/test_wide_cross_seed"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
    assert int(out.stdout.split()[1]) > 100000
