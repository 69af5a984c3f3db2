"""CPU: the premises of the GPU cases of tests/test_gpu_fp32.py (tests/fp32ref.py), with the oracle and a float64
restatement of scale32_pop: a case that stopped holding what it is named for fails here."""
import ctypes

import numpy as np
import pytest

import fp32ref


def test_the_restated_scale_is_the_librarys():
    from clustering_amd import density
    for d in fp32ref.COLS:
        assert fp32ref.k_steps(d) == density.fp32_sweep_plan(1000, d, 1)["k_steps"], d


def test_shapes_cover_every_instance_padding_boundary_and_tile_class():
    steps = {fp32ref.k_steps(d) for d in fp32ref.COLS}
    assert steps == {1, 3, 5, 7, 9, 11, 13, 15, 16}, "every compiled instance meets the oracle"
    assert {d % 2 for d in fp32ref.COLS} == {0, 1}
    assert {4, 5, 8, 9, 16, 17} <= set(fp32ref.COLS) and 3000 > 2 * 16 * 32 * 2 and 257 > 8 * 32
    drawn = {fp32ref.k_steps(d) for _, d, _, _ in fp32ref.fuzz_shapes()}
    assert 11 in drawn and len(fp32ref.fuzz_shapes()) == 40
    assert {k for _, _, k, _ in fp32ref.fuzz_shapes()} >= {1, 2, 8, 9}


@pytest.mark.parametrize("n_cols", (1, 2, 5, 10, 30))
def test_lattice_cases_hold_pairs_exactly_on_a_radius(oracle, n_cols):
    c, radii = fp32ref.lattice_case(n_cols)
    on = fp32ref.lattice_premise(c, radii)
    assert on[1.0] > 0 and on[0.5] > 0, on
    d2 = fp32ref.d2_all(c)
    want = oracle.populations(c, radii)
    for k, r in enumerate(radii):   # strict <: the pairs on the radius are not counted (the self pair is: + 0, d2 = 0 < r2)
        assert (want[k] == (d2 < float(np.float32(r)) ** 2).sum(axis=1)).all(), r


@pytest.mark.parametrize("n_cols", (3, 5, 10, 17, 30))
def test_band_cases_hold_a_band_pair_for_the_smallest_and_the_largest_radius(n_cols):
    c, radii, pairs = fp32ref.band_case(600, n_cols)
    assert radii[0] > radii[1] > radii[2] > 0
    lo, hi = fp32ref.band_premise(c, radii, pairs)
    assert lo < 1.0 and hi < 1.0, (lo, hi)


@pytest.mark.parametrize("n_cols", (2, 5, 9, 30))
def test_tie_cases_hold_duplicates_whose_lowest_index_wins(oracle, n_cols):
    c = fp32ref.tie_case(n_cols)
    assert len(np.unique(c, axis=0)) < len(c) - 250
    fe = np.arange(len(c), 0, -1).astype(np.float32)      # every later row is lower: all of them are candidates
    nn = oracle.nearest_neighbors(c, fe)
    dup = [i for i in range(300, 600) if (c[:40] == c[i]).all(axis=1).any()]
    assert len(dup) == 300
    first = {i: int(np.flatnonzero((c == c[i]).all(axis=1))[0]) for i in dup[:50]}
    assert all(int(nn[0][i]) == j and nn[1][i] == 0.0 for i, j in first.items()), "the lowest index of the equal rows wins"


@pytest.mark.parametrize("n_cols", (5, 10, 30))
def test_tile_test_cases_separate_the_smallest_from_the_largest_radius(oracle, n_cols):
    c, radii = fp32ref.tile_test_case(n_cols)
    assert len(c) > 64, "more than one tile on either side: chains that hold no row twice exist in any order"
    below, above = fp32ref.tile_test_premise(c, radii)
    assert below > 2.0 and above > 2.0, (below, above)
    want = oracle.populations(c, radii)
    assert (want[0] == 1).all() and (want[1] == len(c)).all()


def test_a_frame_whose_population_differs_between_adjacent_radii(oracle):
    for n_cols in (5, 10, 16, 30):
        c = fp32ref.blobs(600, n_cols)
        sets = fp32ref.radius_sets(c)
        want = oracle.populations(c, sets["nine"])
        assert any((want[k] != want[k + 1]).any() for k in range(8)), n_cols
        assert sets["three_equal_pair"][0] == sets["three_equal_pair"][2]
        assert sorted(sets["three_unsorted"]) != sets["three_unsorted"] and [len(v) for v in sets.values()].count(3) == 3
        assert sorted(len(v) for v in sets.values()) == [1, 2, 3, 3, 3, 8, 9]


def test_planted_duplicates():
    for n in (33, 257, 600, 3000):
        c = fp32ref.blobs(n, 5)
        assert (c[0] == c[n - 1]).all() and (c[0] == c[n // 2]).all()
