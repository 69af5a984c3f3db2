"""CPU: the premises of the pruned sweeps' GPU cases at 257..1024 columns (tests/xwidepruneref.py), with a numpy cell order:
the stretched blobs prune at 257, 512 and 1024 columns alike and both counter bounds are equal there, for the population
and for the neighbour sweep; the margin and the cross-block tie cases are what they claim to be at 300 and 1024 columns; the
exact-path bound of the stretched 1 500-row case stays a small share of the evaluated pairs; and the arithmetic the rules
rest on at these widths against long doubles (clustering_amd/bin/test_xwide_prune)."""
import os
import subprocess

import numpy as np
import pytest

import widepruneref as pr
import widennpruneref as nnref
import xwidepruneref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_the_constants_of_these_widths_are_this_modules_own():
    assert ref.F_LO == 1.0 - 7.0e-5 and ref.F_LO < nnref.F_LO, "the 256-column figure does not cover 1024 columns"
    assert (1.0 - 2.0 ** -24) ** (1024 + 2) > ref.F_LO > 1.0 - 1.0e-4
    assert ref.STRETCH == 8 and ref.radii_for(1024)[0] == ref.base_radius(1024)
    assert abs(ref.base_radius(1024) ** 2 - (2 * 0.0064 * 1022 + 2 * 0.4096)) < 1e-9


@pytest.mark.parametrize("n_cols", ref.TABLE_COLS)
@pytest.mark.parametrize("n_rows", sorted(ref.POP_TABLE))
def test_the_population_sweep_prunes_and_both_bounds_are_equal(n_rows, n_cols):
    c = ref.stretched(n_rows, n_cols)
    perm = pr.cell_order(c)
    boxes = pr.block_boxes(c, perm)
    r2max = pr.launch_r2max(ref.radii_for(n_cols))
    assert len(r2max) == 1
    lo, hi = pr.pair_bounds(boxes, r2max[0])
    nb = pr.n_blocks(n_rows)
    assert (lo, nb * nb) == ref.POP_TABLE[n_rows]
    assert lo == hi < nb * nb, "pruning happens, and no block pair lies between the bound and its margin"
    assert pr.tile_bounds(c, perm, ref.radii_for(n_cols)) == (16 * lo, 16 * hi)


def test_the_four_fold_stretch_does_not_prune_at_1024_columns():
    # widepruneref.stretched with its own radii: 512 of 576 tile pairs at 700 rows -- the reason for the data of this module
    c = pr.stretched(700, 1024)
    lo, hi = pr.tile_bounds(c, pr.cell_order(c), pr.radii_for(1024))
    assert lo == hi == 512


@pytest.mark.parametrize("shape", sorted(ref.NN_TABLE))
def test_the_neighbour_sweep_prunes_and_both_bounds_are_equal(shape):
    c, fe = ref.fe_case(*shape)
    perm = pr.cell_order(c)
    lo, hi, s1_lo, s1_hi = ref.nn_pair_bounds(c, fe, perm)
    nb = pr.n_blocks(len(c))
    assert (lo, nb * nb) == ref.NN_TABLE[shape]
    assert lo == hi < nb * nb and s1_lo == s1_hi
    if shape[0] == 2100:
        parts = [ref.nn_pair_bounds(c, fe, perm, s, 3) for s in range(3)]
        assert tuple(sum(p[k] for p in parts) for k in range(4)) == (lo, hi, s1_lo, s1_hi), "segments add up"


def test_mean_populations_at_the_base_radius():
    from oracle.oracle import Oracle
    for n_cols in (257, 1024):
        c = ref.stretched(700, n_cols)
        mean = float(Oracle().populations(c, [ref.base_radius(n_cols)])[0].mean())
        assert 80.0 < mean < 100.0, (n_cols, mean)


@pytest.mark.parametrize("n_cols", [300, 1024])
def test_population_margin_case_premises(oracle, n_cols):
    c, r, (a, b, cc, d) = pr.margin_case(n_cols)
    assert c.shape == (256, n_cols) and r == 3.0
    perm = pr.cell_order(c)
    assert sorted(perm[:128].tolist()) == list(range(0, 256, 2)) and sorted(perm[128:].tolist()) == list(range(1, 256, 2))
    x = c.astype(np.float64)
    d2 = ((x - x[a]) ** 2).sum(axis=1)
    assert d2[d] == (3.0 - 2.0 ** -22) ** 2 < 9.0 and d2[b] == 9.0 and d2[cc] == 9.0 + 2.0 ** -20
    boxes = pr.block_boxes(c, perm)
    assert pr.box_gap2(boxes[:1], boxes[1:])[0, 0] == d2[d], "the box gap of the two blocks IS the pair one ulp inside"
    assert pr.tile_bounds(c, perm, [r]) == (64, 64)
    want = oracle.populations(c, [r])[0]
    assert int(want[a]) == int((d2 < 9.0).sum()) and d2[d] < 9.0


@pytest.mark.parametrize("n_cols", [300, 1024])
def test_cross_block_tie_premises(oracle, n_cols):
    c, fe, (a, p, q) = nnref.cross_block_tie_case(n_cols)
    assert c.shape == (384, n_cols) and q < a < p
    perm = pr.cell_order(c)
    blocks = [set(perm[128 * b:128 * (b + 1)].tolist()) for b in range(3)]
    assert p in blocks[0] and a in blocks[1] and q in blocks[2], "p comes FIRST in the order and has the HIGHER row index"
    x = c.astype(np.float64)
    d2 = ((x - x[a]) ** 2).sum(axis=1)
    rest = np.ones(len(c), dtype=bool)
    rest[[a, p, q]] = False
    assert d2[p] == 9.0 and d2[q] == 9.0 and d2[rest].min() > 9.0 and fe[p] == fe[q] < fe[a]
    nn = oracle.nearest_neighbors(c, fe)
    assert int(nn[0][a]) == q and int(nn[2][a]) == q and nn[1][a] == 9.0 and nn[3][a] == 9.0


@pytest.mark.parametrize("n_cols", [300, 1024])
@pytest.mark.parametrize("which", [-1, 0, 1])
def test_neighbour_margin_case_premises(oracle, which, n_cols):
    c, fe, (a, a2), gap2 = nnref.margin_case(which, n_cols)
    assert c.shape == (384, n_cols)
    perm = pr.cell_order(c)
    groups = [sorted(np.concatenate([np.arange(g, 384, 6), np.arange(g + 1, 384, 6)]).tolist()) for g in (0, 2, 4)]
    for b in range(3):
        assert sorted(perm[128 * b:128 * (b + 1)].tolist()) == groups[b], "each group fills one block"
    boxes = pr.block_boxes(c, perm)
    far2 = nnref.MARGIN_FAR2
    want = {-1: np.nextafter(far2, F32(0)), 0: far2, 1: np.nextafter(far2, F32(100))}[which]
    dx, dy = F32(boxes[2, 0]) - F32(boxes[0, 1]), F32(boxes[2, 2]) - F32(boxes[0, 3])
    assert F32(F32(dx * dx) + F32(dy * dy)) == want == F32(gap2), "one ulp inside, on, one ulp outside far2_nn"
    nn = oracle.nearest_neighbors(c, fe)
    in_a = np.array(groups[0])
    assert int(nn[0][a]) == a2 and nn[1][a] == 9.0 and float(nn[1][in_a].max()) == 9.0
    assert (nn[2] == len(c) + 1).all(), "constant free energies: ring 2 is empty"
    # float64 bounds with the factors of these widths: the block pair lies between f_lo B and f_hi B in all three cases
    assert ref.nn_pair_bounds(c, fe, perm)[:2] == (7, 8)


@pytest.mark.parametrize("n_cols", ref.TABLE_COLS)
def test_the_exact_path_bound_of_the_stretched_case_is_a_small_share(n_cols):
    c = ref.stretched(1500, n_cols)
    lower, _ = pr.tile_bounds(c, pr.cell_order(c), ref.radii_for(n_cols))
    bound = ref.stretched_band_bound(n_cols)
    print(f"D={n_cols}: bound {bound} = {100.0 * bound / (1024 * lower):.2f} % of 1024 x {lower} tile pairs")
    assert lower == 1024
    assert bound <= ref.BAND_SHARE * 1024 * lower


def test_the_arithmetic_of_these_widths_against_long_doubles():
    exe = os.path.join(ROOT, "clustering_amd", "bin", "test_xwide_prune")
    assert os.path.exists(exe), "build() makes clustering_amd/bin/test_xwide_prune"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
    assert int(out.stdout.split()[1]) > 100000
