"""GPU: the pruned cross neighbour sweep at 257..1024 columns (density.nearest_reference_xwide_pruned) against the referee of
tests/test_gpu_cross_wide.py -- the probe's canonical d2 of the [n_q, n_r] block in the library's summation order, the least
(d2, row), the IEEE comparison of free energies (tests/crossref.py) --, bit for bit on all four arrays, and against the
unpruned dc_hip_nearest_neighbors_cross_xwide_dev call.  Every finite, non-empty case asserts the counter condition: with
everything formed in float64 from the device's own two orders (xwide_against_pruned_order) and the seed premise re-asserted
on them, 16 |lower| <= tiles <= 16 |upper| and mfmas == tiles x ceil((2 + 3 D) / 16).  Cases and bounds:
tests/xcrosswidepruneref.py (their premises are checked on the CPU by tests/test_cross_xwide_pruned_cases.py)."""
import functools

import numpy as np
import pytest

import crossref
import xcrosswidepruneref as ref
from crossref import FLT_MAX, block_d2, expect_nn, gpu, host, same_nn

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def dens():
    import torch
    assert torch.cuda.is_available()
    from clustering_amd import density
    return density


@functools.lru_cache(maxsize=None)
def the_probe():
    from clustering_amd import capi
    from oracle.oracle import Probe
    return Probe(capi.CANON_ORDER)


@functools.lru_cache(maxsize=None)
def split_case(n_q, n_r, n_cols):
    """(Q, R, fe_q, fe_r, d2) of the split stretched blobs: computed once per shape"""
    Q, R, fe_q, fe_r = ref.split_case(n_q, n_r, n_cols)
    return Q, R, fe_q, fe_r, block_d2(the_probe(), Q, R)


def run(dens, Q, R, fe_q, fe_r, lo=0, hi=None, want=None):
    """one call on finite data with something to sweep -> (the four arrays, (tiles, mfmas, exact), (perm_q, perm_r), (lower,
    upper) of the tile counter).  Values first -- against want and against the unpruned call --, then the counters"""
    q, r = gpu(Q), gpu(R)
    hi = len(Q) if hi is None else hi
    with_fe = fe_q is not None
    fq, fr = (gpu(fe_q), gpu(fe_r)) if with_fe else (None, None)
    got = dens.nearest_reference_xwide_pruned(q, r, fq, fr, lo, hi)
    tiles, mfmas, exact = dens.xwide_against_pruned_info(q.device)
    perm_q, perm_r = (p.cpu().numpy().astype(np.int64) for p in dens.xwide_against_pruned_order(q.device))
    if want is not None:
        same_nn(got, want, (Q.shape, R.shape, lo, hi, with_fe))
    plain = dens.nearest_reference_xwide(q, r, fq, fr, lo, hi)
    for a, b in zip(got, plain):
        assert (a is None and b is None) or (host(a).view(np.uint32) == host(b).view(np.uint32)).all(), "the unpruned call's"
    if not with_fe:
        assert got[2] is None and got[3] is None, "no free energies: no hd arrays"
    assert sorted(perm_q.tolist()) == list(range(lo, hi)), "the query order is a permutation of the rows of the range"
    assert sorted(perm_r.tolist()) == list(range(len(R))), "the reference order is a permutation of its rows"
    lower, upper = ref.nn_tile_bounds(Q, R, fe_q, fe_r, perm_q, perm_r)   # (asserts the seed premise on the device's orders)
    n_pairs = ref.query_blocks(lo, hi) * ref.n_blocks(len(R))
    print(f"{Q.shape} x {R.shape} [{lo}, {hi}) fe={with_fe}: tiles {tiles} in [{lower}, {upper}], all {16 * n_pairs}, exact pairs {exact}")
    assert tiles >= 16 * ref.query_blocks(lo, hi) and mfmas > 0, "the matrix-core kernel did not answer: a seed block pair per query block at least"
    assert mfmas == ref.mfmas_per_tile_pair(Q.shape[1]) * tiles, (tiles, mfmas)
    assert lower <= tiles <= upper <= 16 * n_pairs, "the counter condition"
    return got, (tiles, mfmas, exact), (perm_q, perm_r), (lower, upper)


def check(dens, Q, R, d2, fe_q, fe_r, lo=0, hi=None):
    return run(dens, Q, R, fe_q, fe_r, lo, hi, want=expect_nn(d2, fe_q, fe_r, lo, hi))


@pytest.mark.parametrize("n_q,n_r,n_cols", sorted(ref.NN_TABLE))
def test_the_split_shapes_prune_to_the_tables_figures(dens, n_q, n_r, n_cols):
    Q, R, fe_q, fe_r, d2 = split_case(n_q, n_r, n_cols)
    with_fe, nn_only = ref.NN_TABLE[(n_q, n_r, n_cols)]
    _, (tiles, _, exact), _, (lower, upper) = check(dens, Q, R, d2, fe_q, fe_r)
    assert upper < 16 * ref.n_blocks(n_q) * ref.n_blocks(n_r), "pruning happened"
    print(f"D={n_cols}: {exact} exact pairs = {100.0 * exact / (1024 * tiles):.3f} % of the evaluated pairs")
    assert exact <= ref.NN_EXACT_SHARE * 1024 * tiles, "the exact path's share"
    if lower == upper:   # (the CPU premise under the numpy order; under the device's order the counter is then pinned)
        assert tiles == 16 * with_fe, (tiles, lower)
    # fe_query=None: no hd arrays, no ring 2
    got, (tiles, _, _), _, (lower, upper) = check(dens, Q, R, d2, None, None)
    if lower == upper:
        assert tiles == 16 * nn_only, (tiles, lower)


@pytest.mark.parametrize("n_cols", ref.COLS)
def test_column_counts(dens, n_cols):
    Q, R, fe_q, fe_r, d2 = split_case(300, 1500, n_cols)
    check(dens, Q, R, d2, fe_q, fe_r)


@pytest.mark.parametrize("n_q,n_r", [(1, 300), (127, 300), (128, 300), (129, 300), (1500, 1)])
def test_query_counts_around_a_block_and_a_reference_of_one_row(dens, n_q, n_r):
    Q, R, fe_q, fe_r, d2 = split_case(n_q, n_r, 300)
    got, _, _, _ = check(dens, Q, R, d2, fe_q, fe_r)
    assert bool((got[0] != n_r + 1).all()), "every query has a nearest reference"
    check(dens, Q, R, d2, None, None)


@pytest.mark.parametrize("lo,hi", [(37, 171), (128, 256), (0, 1), (299, 300), (127, 129)])
def test_a_row_range_inside_a_larger_query_array(dens, lo, hi):
    Q, R, fe_q, fe_r, d2 = split_case(300, 1500, 300)
    got, _, _, _ = check(dens, Q, R, d2, fe_q, fe_r, lo, hi)
    outside = np.ones(300, dtype=bool)
    outside[lo:hi] = False
    for k in (0, 2):
        assert (host(got[k])[outside] == len(R) + 1).all() and (host(got[k + 1])[outside] == FLT_MAX).all(), "none outside the range"
        assert (host(got[k])[~outside] != len(R) + 1).any()


@pytest.mark.parametrize("n_cols", [300, 1024])
def test_the_margin_at_its_sharpest(dens, n_cols):
    """a reference block whose gap is one ulp below, on, and one ulp above far2_nn: met, not met, not met"""
    tiles = {}
    for which in (-1, 0, 1):
        Q, R, fe_q, fe_r, a_q, gap2 = ref.nn_margin_sets(which, n_cols)
        d2 = block_d2(the_probe(), Q, R)
        got, info, (perm_q, perm_r), bounds = check(dens, Q, R, d2, fe_q, fe_r)
        for b in range(3):
            assert sorted(perm_r[128 * b:128 * (b + 1)].tolist()) == list(range(b, 384, 3)), "the premise: each group fills one block"
        assert bounds == (32, 48) and float(got[1][a_q]) == 9.0 and float(host(got[1]).max()) == 9.0
        assert bool((got[2] == len(R) + 1).all()), "constant free energies: ring 2 is empty"
        tiles[which] = info[0]
    assert tiles == {-1: 48, 0: 32, 1: 32}, "the seed block and M always; the far block only with its gap below far2_nn"


def test_copies_of_reference_rows_find_them_at_distance_zero(dens):
    Q, R, copies = ref.duplicate_sets()
    d2 = block_d2(the_probe(), Q, R)
    rng = np.random.default_rng(5)
    fe_q, fe_r = rng.normal(size=len(Q)).astype(np.float32), rng.normal(size=len(R)).astype(np.float32)
    got, _, _, _ = check(dens, Q, R, d2, fe_q, fe_r)
    dup = copies >= 0
    assert (host(got[1])[dup] == 0).all() and (host(got[0])[dup] == copies[dup]).all(), "d2 = 0, the row it copies"
    assert (host(got[1])[~dup] > 0).all()


def test_queries_far_from_the_whole_reference_still_have_a_seed(dens):
    Q, R, fe_q, fe_r = ref.far_sets()
    d2 = block_d2(the_probe(), Q, R)
    got, info, _, _ = check(dens, Q, R, d2, fe_q, fe_r)
    assert bool((got[0] != len(R) + 1).all()) and bool((got[1] < FLT_MAX).all()), "every query has a nearest reference"
    assert info[0] >= 16 * ref.n_blocks(len(Q)), "the seed block pairs at least"


def test_a_tie_across_reference_blocks_goes_to_the_lower_row(dens):
    Q, R, fe_q, fe_r, (a_q, p, q) = ref.cross_block_tie_sets(300)
    d2 = block_d2(the_probe(), Q, R)
    got, _, (perm_q, perm_r), _ = check(dens, Q, R, d2, fe_q, fe_r)
    pos = {int(row): k for k, row in enumerate(perm_r)}
    assert pos[p] // 128 == 0 and pos[q] // 128 == 2 and q < p, "the premise, from the device's order: the lower row sits in the last block"
    assert d2[a_q, p] == F32(9.0) and d2[a_q, q] == F32(9.0)
    for k in (0, 2):
        assert int(got[k][a_q]) == q and float(got[k + 1][a_q]) == 9.0, "the least (d2, ROW): a merge on positions would answer p"


def test_a_query_block_at_or_below_the_references_least_has_no_ring_2(dens):
    Q, R, _, _, d2 = split_case(700, 2100, 257)
    zq, zr = np.zeros(len(Q), dtype=np.float32), np.zeros(len(R), dtype=np.float32)
    _, nn_only, perms, _ = check(dens, Q, R, d2, None, None)
    for fe_q in (zq, zq - F32(1.0)):
        got, info, _, (lower, upper) = check(dens, Q, R, d2, fe_q, zr)
        assert bool((got[2] == len(R) + 1).all()) and bool((got[3] == FLT_MAX).all())
        assert (lower, upper) == ref.nn_tile_bounds(Q, R, None, None, *perms), "the bounds of the seed launch and ring 1 alone"
        assert info[0] == nn_only[0], "ring 2 met no block: the tile pairs of the nn-only call"


@pytest.mark.parametrize("n_cols", [300, 512])   # (beyond 400 columns the column-chunked direct kernel answers)
@pytest.mark.parametrize("flaw", ["nan query", "inf reference", "nan fe_ref", "nan fe_query"])
def test_flagged_data_is_answered_by_the_direct_kernel(dens, flaw, n_cols):
    Q0, R0, fq0, fr0, d20 = split_case(300, 1500, n_cols)
    Q, R, fe_q, fe_r = Q0.copy(), R0.copy(), fq0.copy(), fr0.copy()
    kind, side = flaw.split()
    if side.startswith("fe_"):
        (fe_q if side == "fe_query" else fe_r)[131] = np.nan
        d2 = d20
    else:
        X = Q if side == "query" else R
        X[{"nan": 131, "inf": 40}[kind], {"nan": 7, "inf": n_cols - 1}[kind]] = {"nan": np.nan, "inf": np.inf}[kind]
        assert crossref.stats_flagged(Q, R)
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = block_d2(the_probe(), Q, R)
    q, r, fq, fr = gpu(Q), gpu(R), gpu(fe_q), gpu(fe_r)
    for lo, hi in ((0, 300), (37, 171)):
        got = dens.nearest_reference_xwide_pruned(q, r, fq, fr, lo, hi)
        assert dens.xwide_against_pruned_info(q.device) == (0, 0, 0)
        plain = dens.nearest_reference_xwide(q, r, fq, fr, lo, hi)
        for a, b in zip(got, plain):
            assert (host(a).view(np.uint32) == host(b).view(np.uint32)).all(), "the unpruned call's"
        same_nn(got, expect_nn(d2, fe_q, fe_r, lo, hi), flaw)
    # a NaN outside the query range flags nothing; one in the reference's always does
    if flaw == "nan fe_query":
        got = dens.nearest_reference_xwide_pruned(q, r, fq, fr, 140, 300)
        assert dens.xwide_against_pruned_info(q.device)[0] > 0, "the NaN is outside the range"
        same_nn(got, expect_nn(d2, fe_q, fe_r, 140, 300), "the NaN is outside the range")
    # ... and a clean call behind it in the same workspace runs on the matrix cores again
    check(dens, Q0, R0, d20, fq0, fr0)


def test_a_small_call_behind_a_large_one_and_both_sweeps_alternating_in_one_workspace(dens):
    big, small = split_case(1100, 8320, 257), split_case(1, 300, 300)
    check(dens, big[0], big[1], big[4], big[2], big[3])
    check(dens, small[0], small[1], small[4], small[2], small[3])
    Q, R, fe_q, fe_r, d2 = split_case(300, 1500, 1024)
    radii = ref.radii_for(1024)
    q, r = gpu(Q), gpu(R)
    for _ in range(2):
        pops = dens.calculate_populations_against_xwide_pruned(q, r, radii, 37, 171)
        assert (host(pops) == crossref.expect_pops(d2, radii, 37, 171)).all()
        perm_q, _ = dens.xwide_against_pruned_order(q.device)
        assert sorted(perm_q.tolist()) == list(range(37, 171))
        check(dens, Q, R, d2, fe_q, fe_r)
        perm_q, perm_r = dens.xwide_against_pruned_order(q.device)   # the order after a neighbour call: the call's own
        assert sorted(perm_q.tolist()) == list(range(300)) and sorted(perm_r.tolist()) == list(range(1500))
    check(dens, Q, R, d2, fe_q, fe_r, 127, 129)


@pytest.mark.parametrize("pruned_neighbours", [False, True])
def test_assign_frames_xwide_pruned_equals_assign_frames_xwide_in_every_entry(dens, pruned_neighbours):
    import torch
    n_q, n_r, D = 300, 1500, 300
    Q, R = ref.split_sets(n_q, n_r, D)
    states_r = (np.arange(n_r) % 5 + 1).astype(np.int32)
    q, r = gpu(Q), gpu(R)
    want = dens.assign_frames_xwide(q, r, ref.base_radius(D), states_r)
    got = dens.assign_frames_xwide_pruned(q, r, ref.base_radius(D), states_r, pruned_neighbours=pruned_neighbours)
    tiles, mfmas, _ = dens.xwide_against_pruned_info(q.device)
    assert 0 < tiles < 16 * ref.n_blocks(n_q) * ref.n_blocks(n_r) and mfmas == ref.mfmas_per_tile_pair(D) * tiles, "the pruned sweep answered"
    assert dens.xwide_pruned_info(q.device)[0] > 0, "the reference's own populations through the pruned self sweep"
    assert set(got) == set(want)
    for key, val in want.items():
        if key == "max_pop":
            assert got[key] == val
        else:
            assert got[key].dtype == val.dtype and got[key].shape == val.shape, key
            assert bool((got[key].view(torch.int32) == val.view(torch.int32)).all()), (key, pruned_neighbours)
    assert int((got["states"] == 0).sum()) == 0
