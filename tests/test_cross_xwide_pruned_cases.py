"""CPU: the premises of the pruned cross sweeps' GPU cases at 257..1024 columns (tests/xcrosswidepruneref.py), with the numpy
joint-grid order: the split stretched blobs prune alike at 257, 512 and 1024 columns and both counter bounds are equal
there, for the population and for the neighbour sweep (with its seed premise); the exact-path cap of the 1 500 x 1 500 case
is the recorded pair count and a small share of the evaluated pairs; the edge cases are what they claim to be at these
widths; and the arithmetic the rules rest on for two boxes against long doubles (clustering_amd/bin/test_xwide_cross_prune)."""
import os
import subprocess

import numpy as np
import pytest

import crosswidennpruneref as cn
import crosswidepruneref as cp
import widepruneref as pr
import xcrosswidepruneref as ref
import xwidepruneref as xp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
POP_SHAPES = [(n_q, n_r, d) for (n_q, n_r), cols in sorted(ref.POP_COLS.items()) for d in cols]


def test_the_constants_are_those_of_these_widths():
    assert ref.F_LO == xp.F_LO == 1.0 - 7.0e-5 < cn.F_LO and ref.F_HI == xp.F_HI == 1.001
    assert ref.FLOOR == 2.0 ** -122 == 16 * cn.FLT_MIN and ref.BAND_SHARE == xp.BAND_SHARE == 0.08
    assert ref.COLS == xp.COLS and ref.stretched is xp.stretched and ref.radii_for is xp.radii_for
    assert ref.joint_order is cp.joint_order and ref.gaps is cp.gaps and ref.tile_bounds is cp.tile_bounds
    assert sorted(POP_SHAPES) == sorted(ref.NN_TABLE), "the two tables cover the same shapes"
    Q, R = ref.split_sets(300, 1500, 257)
    c = xp.stretched(1800, 257)
    assert (Q == c[:300]).all() and (R == c[300:]).all(), "the first n_q rows are the queries, the rest the reference"


@pytest.mark.parametrize("n_q,n_r,n_cols", POP_SHAPES)
def test_the_population_sweep_prunes_and_both_bounds_are_equal(n_q, n_r, n_cols):
    Q, R = ref.split_sets(n_q, n_r, n_cols)
    perm_q, perm_r = ref.joint_order(Q, R)
    g = ref.gaps(Q, R, perm_q, perm_r)
    r2max = pr.launch_r2max(ref.radii_for(n_cols))
    assert len(r2max) == 1
    lo, hi = cp.pair_bounds(g, r2max[0])
    assert (lo, g.size) == ref.POP_TABLE[(n_q, n_r)]
    assert lo == hi < g.size, "pruning happens, and no block pair lies between the bound and its margin"
    assert ref.tile_bounds(Q, R, perm_q, perm_r, ref.radii_for(n_cols)) == (16 * lo, 16 * hi)
    assert g.shape == (ref.n_blocks(n_q), ref.n_blocks(n_r))


@pytest.mark.parametrize("shape", sorted(ref.NN_TABLE))
def test_the_neighbour_sweep_prunes_and_both_bounds_are_equal(shape):
    Q, R, fe_q, fe_r = ref.split_case(*shape)
    assert np.isfinite(fe_q).all(), "every query has a reference inside the radius"
    perm_q, perm_r = ref.joint_order(Q, R)
    all_pairs = ref.n_blocks(shape[0]) * ref.n_blocks(shape[1])
    with_fe, nn_only = ref.NN_TABLE[shape]
    lo, hi, s1_lo, s1_hi = ref.nn_pair_bounds(Q, R, fe_q, fe_r, perm_q, perm_r)   # (asserts the seed premise)
    assert lo == hi == with_fe < all_pairs and s1_lo == s1_hi == nn_only
    assert ref.nn_pair_bounds(Q, R, None, None, perm_q, perm_r) == (nn_only,) * 4
    assert ref.nn_tile_bounds(Q, R, fe_q, fe_r, perm_q, perm_r) == (16 * with_fe, 16 * with_fe)


@pytest.mark.parametrize("n_cols", sorted(ref.BAND_PAIRS))
def test_the_exact_path_cap_of_the_population_sweep_is_a_small_share(n_cols):
    Q, R = ref.split_sets(1500, 1500, n_cols)
    lower, _ = ref.tile_bounds(Q, R, *ref.joint_order(Q, R), ref.radii_for(n_cols))
    assert lower == 16 * 64
    count = ref.band_pairs(n_cols)
    print(f"D={n_cols}: {count} pairs inside the band = {100.0 * count / (1024 * lower):.2f} % of 1024 x {lower} tile pairs")
    assert count == ref.BAND_PAIRS[n_cols]
    assert count <= ref.BAND_SHARE * 1024 * lower


@pytest.mark.parametrize("n_cols", [300, 1024])
def test_population_margin_sets_premises(n_cols):
    Q, R, r, (a, b, c, d) = ref.margin_sets(n_cols)
    assert Q.shape == R.shape == (128, n_cols) and r == 3.0
    perm_q, perm_r = ref.joint_order(Q, R)
    g = ref.gaps(Q, R, perm_q, perm_r)
    d2 = ((Q[a].astype(np.float64)[None, :] - R.astype(np.float64)) ** 2).sum(axis=1)
    assert d2[d] == (3.0 - 2.0 ** -22) ** 2 < 9.0 and d2[b] == 9.0 and d2[c] == 9.0 + 2.0 ** -20
    assert g.shape == (1, 1) and g[0, 0] == d2[d], "the box gap of the two blocks IS the pair one ulp inside"
    assert ref.tile_bounds(Q, R, perm_q, perm_r, [r]) == (16, 16)


@pytest.mark.parametrize("n_cols", [300, 1024])
@pytest.mark.parametrize("which", [-1, 0, 1])
def test_neighbour_margin_sets_premises(which, n_cols):
    Q, R, fe_q, fe_r, a_q, gap2 = ref.nn_margin_sets(which, n_cols)
    assert Q.shape == (128, n_cols) and R.shape == (384, n_cols)
    perm_q, perm_r = ref.joint_order(Q, R)
    for b in range(3):
        assert sorted(perm_r[128 * b:128 * (b + 1)].tolist()) == list(range(b, 384, 3)), "each group fills one block"
    boxes_q, boxes_r = pr.block_boxes(Q, perm_q), pr.block_boxes(R, perm_r)
    far2 = cn.MARGIN_FAR2
    want = {-1: np.nextafter(far2, F32(0)), 0: far2, 1: np.nextafter(far2, F32(100))}[which]
    dx, dy = F32(boxes_r[2, 0]) - F32(boxes_q[0, 1]), F32(boxes_r[2, 2]) - F32(boxes_q[0, 3])
    assert F32(F32(dx * dx) + F32(dy * dy)) == want == F32(gap2), "one ulp inside, on, one ulp outside far2_nn"
    # float64 bounds with the factors of these widths: the far block lies between F_LO B and F_HI B in all three cases
    assert ref.nn_pair_bounds(Q, R, fe_q, fe_r, perm_q, perm_r)[:2] == (2, 3)
    counts, bounds = ref.block_counts(Q, R, fe_q, fe_r, perm_q, perm_r)
    assert abs(bounds[0, 0] - 9.0) < 1e-9, "the bound of the query block after its seed launch (float64, Gram form)"


def test_cross_block_tie_sets_premises():
    Q, R, fe_q, fe_r, (a_q, p, q) = ref.cross_block_tie_sets(300)
    assert Q.shape[1] == R.shape[1] == 300 and q < p
    _, perm_r = ref.joint_order(Q, R)
    pos = {int(row): k for k, row in enumerate(perm_r)}
    assert pos[p] // 128 == 0 and pos[q] // 128 == 2, "the lower row sits in the block the order puts last"
    d2 = ((Q[a_q].astype(np.float64)[None, :] - R.astype(np.float64)) ** 2).sum(axis=1)
    rest = np.ones(len(R), dtype=bool)
    rest[[p, q]] = False
    assert d2[p] == 9.0 and d2[q] == 9.0 and d2[rest].min() > 9.0 and fe_r[p] == fe_r[q] < fe_q[a_q]


def test_duplicate_far_and_unpruned_sets_premises():
    Q, R, copies = ref.duplicate_sets()
    dup = np.flatnonzero(copies >= 0)
    assert len(dup) == 30 and (Q[dup] == R[copies[dup]]).all()
    d2 = ref.cross_d2(Q, R)
    others = np.flatnonzero(copies < 0)
    assert d2[others].min() > 1e-3, "no other pair comes near: at r = 1e-20 the populations are the duplicate counts"
    r2 = F32(ref.TINY_RADIUS) * F32(ref.TINY_RADIUS)
    assert 0.0 < float(r2) < float(np.finfo(np.float32).tiny) < ref.FLOOR, "fl32(r^2) is subnormal, below the floor"
    Qf, Rf, _, _ = ref.far_sets()
    gf = ref.gaps(Qf, Rf, *ref.joint_order(Qf, Rf))
    assert gf.min() > 1000.0 * max(pr.launch_r2max(ref.radii_for(300))), "far from every reference block"
    for n_cols in (257, 1024):
        Qu, Ru, radii = ref.unpruned_sets(n_cols)
        lo, hi = ref.tile_bounds(Qu, Ru, *ref.joint_order(Qu, Ru), radii)
        assert lo == hi == 16 * ref.n_blocks(len(Qu)) * ref.n_blocks(len(Ru)) == 16 * 4 * 8, "nothing to prune"


def test_the_arithmetic_of_two_boxes_against_long_doubles():
    exe = os.path.join(ROOT, "clustering_amd", "bin", "test_xwide_cross_prune")
    assert os.path.exists(exe), "build() makes clustering_amd/bin/test_xwide_cross_prune"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
    assert int(out.stdout.split()[1]) > 20000
