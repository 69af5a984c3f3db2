"""GPU: the pruned wide cross neighbour sweep (density.nearest_reference_wide_pruned, 65..256 columns) against the referee
of tests/test_gpu_cross_wide.py -- the probe's canonical d2 of the [n_q, n_r] block, the least (d2, row), the IEEE
comparison of free energies (tests/crossref.py) --, bit for bit on all four arrays.  Every finite, non-empty case first
asserts that the matrix-core kernel answered (wide_against_pruned_info: mfmas_per_tile_pair(D) MFMAs per tile pair) and then
the counter condition: with everything formed in float64 from the device's own two orders (wide_against_pruned_order) and
the seed premise re-asserted on them, 16 |lower| <= tiles <= 16 |upper|.  Cases and bounds: tests/crosswidennpruneref.py
(their premises are checked on the CPU by tests/test_cross_wide_nn_pruned_cases.py)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import crossref
import crosswidennpruneref as ref
import crosswidepruneref as cp
import fe_families
from crossref import FLT_MAX, block_d2, expect_nn, gpu, host, same_nn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def run(dens, Q, R, fe_q, fe_r, lo=0, hi=None, q=None, r=None):
    """one call on finite data with something to sweep -> (the four arrays, (tiles, mfmas, exact), (perm_q, perm_r), (lower,
    upper) of the tile counter); asserts the counters"""
    q = gpu(Q) if q is None else q
    r = gpu(R) if r is None else r
    hi = len(Q) if hi is None else hi
    with_fe = fe_q is not None
    got = dens.nearest_reference_wide_pruned(q, r, gpu(fe_q) if with_fe else None, gpu(fe_r) if with_fe else None, lo, hi)
    tiles, mfmas, exact = dens.wide_against_pruned_info(q.device)
    perm_q, perm_r = (p.cpu().numpy().astype(np.int64) for p in dens.wide_against_pruned_order(q.device))
    assert sorted(perm_q.tolist()) == list(range(lo, hi)), "the query order is a permutation of the rows of the range"
    assert sorted(perm_r.tolist()) == list(range(len(R))), "the reference order is a permutation of its rows"
    lower, upper = ref.tile_bounds(Q, R, fe_q, fe_r, perm_q, perm_r)   # (asserts the seed premise on the device's orders)
    n_pairs = cp.query_blocks(lo, hi) * cp.n_blocks(len(R))
    print(f"{Q.shape} x {R.shape} [{lo}, {hi}) fe={with_fe}: tiles {tiles} in [{lower}, {upper}], all {16 * n_pairs}, exact pairs {exact}")
    assert tiles >= 16 * cp.query_blocks(lo, hi) and mfmas > 0, "the matrix-core kernel did not answer: a seed block pair per query block at least"
    assert mfmas == ref.mfmas_per_tile_pair(Q.shape[1]) * tiles, (tiles, mfmas)
    assert lower <= tiles <= upper <= 16 * n_pairs, "the counter condition"
    if not with_fe:
        assert got[2] is None and got[3] is None
    return got, (tiles, mfmas, exact), (perm_q, perm_r), (lower, upper)


def check(dens, Q, R, d2, fe_q, fe_r, lo=0, hi=None, what=""):
    got, info, perms, bounds = run(dens, Q, R, fe_q, fe_r, lo, hi)
    same_nn(got, expect_nn(d2, fe_q, fe_r, lo, hi), (what, Q.shape, R.shape, lo, hi))
    return got, info, perms, bounds


@pytest.mark.parametrize("n_cols", [65, 84, 85, 128, 256])
def test_column_counts(dens, n_cols):
    Q, R, fe_q, fe_r, d2 = split_case(300, 1500, n_cols)
    check(dens, Q, R, d2, fe_q, fe_r)


@pytest.mark.parametrize("n_q,n_r,n_cols", [(1, 300, 100), (300, 1, 100), (33, 129, 100), (129, 33, 100), (300, 1500, 100),
                                            (1500, 300, 100), (1500, 1500, 65), (1500, 1500, 256), (700, 2100, 100),
                                            (1100, 8320, 80)])
def test_rectangles_in_both_orientations_and_every_padding(dens, n_q, n_r, n_cols):
    # 1 500 x 300: more query blocks than the reference has blocks at all; 700 x 2 100: 17 reference blocks in two shares;
    # 1 100 x 8 320: 65 in eight, past one share per block
    Q, R, fe_q, fe_r, d2 = split_case(n_q, n_r, n_cols)
    _, (tiles, _, _), _, (lower, upper) = check(dens, Q, R, d2, fe_q, fe_r)
    if (n_q, n_r, n_cols) in ref.SPLIT_TABLE:
        assert upper < 16 * cp.n_blocks(n_q) * cp.n_blocks(n_r), "pruning happened"
        if lower == upper:   # (the CPU premise under the numpy order; under the device's order the counter is then pinned)
            assert tiles == lower == 16 * ref.SPLIT_TABLE[(n_q, n_r, n_cols)][0], (tiles, lower)
    check(dens, Q, R, d2, None, None, what="nn only")


@pytest.mark.parametrize("lo,hi", [(37, 171), (128, 256), (0, 1), (299, 300), (127, 129)])
def test_row_ranges_that_start_and_end_inside_tiles_and_blocks(dens, lo, hi):
    Q, R, fe_q, fe_r, d2 = split_case(300, 1500, 100)
    got, _, _, _ = check(dens, Q, R, d2, fe_q, fe_r, lo, hi)
    outside = np.ones(300, dtype=bool)
    outside[lo:hi] = False
    for k in (0, 2):
        assert (host(got[k])[outside] == len(R) + 1).all() and (host(got[k + 1])[outside] == FLT_MAX).all(), "none outside the range"


def test_an_empty_side_and_an_empty_range_give_none_and_sweep_nothing(dens):
    import torch
    Q0, R0, fq0, fr0, d20 = split_case(33, 129, 100)
    for n_q, n_r in ((40, 0), (0, 40), (0, 0)):
        check(dens, Q0, R0, d20, fq0, fr0)   # (a call before it leaves counters behind that the empty call must not keep)
        q = torch.zeros((n_q, 100), dtype=torch.float32, device="cuda")
        r = torch.zeros((n_r, 100), dtype=torch.float32, device="cuda")
        fe_q, fe_r = torch.zeros(n_q, device="cuda"), torch.zeros(n_r, device="cuda")
        for with_fe in (False, True):
            nn = dens.nearest_reference_wide_pruned(q, r, fe_q if with_fe else None, fe_r if with_fe else None)
            assert dens.wide_against_pruned_info(q.device) == (0, 0, 0)
            for idx, dd in ((nn[0], nn[1]),) + (((nn[2], nn[3]),) if with_fe else ()):
                assert idx.shape == (n_q,) and bool((idx == n_r + 1).all()) and bool((dd == FLT_MAX).all())
    check(dens, Q0, R0, d20, fq0, fr0)
    nn = dens.nearest_reference_wide_pruned(gpu(Q0), gpu(R0), gpu(fq0), gpu(fr0), 5, 5)
    assert dens.wide_against_pruned_info(nn[0].device) == (0, 0, 0)
    for k in (0, 2):
        assert bool((nn[k] == len(R0) + 1).all()) and bool((nn[k + 1] == FLT_MAX).all())


@pytest.mark.parametrize("family", sorted(fe_families.FAMILIES))
def test_free_energies_of_any_origin_on_both_sides(dens, family):
    Q, R, _, _, d2 = split_case(300, 1500, 100)
    pops_q, pops_r = ref.pops_pair(Q, R, ref.std_radius(100))
    fe_q, fe_r = fe_families.make(family, Q, pops_q, seed=3), fe_families.make(family, R, pops_r, seed=4)
    if family == "nan":   # flagged: the direct kernel answers, with the same IEEE comparison
        got = dens.nearest_reference_wide_pruned(gpu(Q), gpu(R), gpu(fe_q), gpu(fe_r))
        assert dens.wide_against_pruned_info(got[0].device) == (0, 0, 0)
        same_nn(got, expect_nn(d2, fe_q, fe_r), family)
    else:
        check(dens, Q, R, d2, fe_q, fe_r, what=family)


def test_infinite_and_signed_zero_free_energies_across_the_sets(dens):
    Q, R, _, fe_r, d2 = split_case(300, 1500, 100)
    n_q, n_r = len(Q), len(R)
    full = lambda n, v: np.full(n, v, dtype=np.float32)
    # -0 is not below +0, either way round: no lower reference, ring 2 is empty
    for vq, vr in ((-0.0, 0.0), (0.0, -0.0)):
        got, info, _, _ = check(dens, Q, R, d2, full(n_q, vq), full(n_r, vr), what=("zeros", vq, vr))
        assert bool((got[2] == n_r + 1).all())
    got, _, _, _ = check(dens, Q, R, d2, full(n_q, np.inf), fe_r, what="fe_query +inf")
    assert bool((got[2] == got[0]).all()), "everything finite lies below +inf: nn_hd is nn"
    got, _, _, _ = check(dens, Q, R, d2, full(n_q, -np.inf), fe_r, what="fe_query -inf")
    assert bool((got[2] == n_r + 1).all()), "nothing lies below -inf"
    check(dens, Q, R, d2, full(n_q, 0.0), full(n_r, -np.inf), what="fe_ref -inf")
    check(dens, Q, R, d2, full(n_q, 0.0), full(n_r, np.inf), what="fe_ref +inf")


def test_a_query_block_at_or_below_the_references_least_has_no_ring_2(dens):
    Q, R, _, _, d2 = split_case(700, 2100, 100)
    zq, zr = np.zeros(len(Q), dtype=np.float32), np.zeros(len(R), dtype=np.float32)
    _, nn_only, perms, _ = check(dens, Q, R, d2, None, None, what="nn only")
    for fe_q in (zq, zq - F32(1.0)):
        got, info, _, (lower, upper) = check(dens, Q, R, d2, fe_q, zr, what="no lower reference")
        assert bool((got[2] == len(R) + 1).all()) and bool((got[3] == FLT_MAX).all())
        assert (lower, upper) == ref.tile_bounds(Q, R, None, None, *perms), "the bounds of the seed launch and ring 1 alone"
        assert info[0] == nn_only[0], "ring 2 met no block"


def test_a_query_without_a_lower_reference_meets_every_block_that_holds_a_lower_row(dens):
    Q, R, _, _, d2 = split_case(700, 2100, 100)
    gq, gr = ref.shifted_gradient(Q, R)
    got, info, (perm_q, perm_r), (lower, upper) = check(dens, Q, R, d2, gq, gr, what="gradient")
    counts, bounds = ref.block_counts(Q, R, gq, gr, perm_q, perm_r)
    assert np.isinf(bounds[:, 1]).any() and bool((got[2] == len(R) + 1).any()), "the premise, from the device's orders"
    assert lower > ref.tile_bounds(Q, R, None, None, perm_q, perm_r)[1], "ring 2 adds block pairs"


def test_duplicates_between_and_within_the_sets(dens):
    Q, R = crossref.sets(100, 300, 700, seed=19)
    d2 = block_d2(the_probe(), Q, R)
    assert int((d2 == 0).sum()) > 0
    rng = np.random.default_rng(5)
    fe_q, fe_r = rng.normal(size=len(Q)).astype(np.float32), rng.normal(size=len(R)).astype(np.float32)
    got, _, _, _ = check(dens, Q, R, d2, fe_q, fe_r, what="duplicates")
    dup = (d2 == 0).any(axis=1)
    assert (host(got[1])[dup] == 0).all() and (host(got[0])[dup] == np.argmax(d2 == 0, axis=1)[dup]).all(), "d2 = 0, the lowest row"


def test_queries_and_reference_in_the_same_array(dens):
    """Q == R, the same tensor: an ordinary pair of sets -- every frame finds itself at d2 = 0"""
    import torch
    c = ref.pr.stretched(1100, 100)
    d2 = block_d2(the_probe(), c, c)
    ct = torch.from_numpy(c).cuda()
    fe = np.ascontiguousarray(c[:, 2])
    got, _, (perm_q, perm_r), _ = run(dens, c, c, fe, fe, q=ct, r=ct)
    same_nn(got, expect_nn(d2, fe, fe), "Q == R")
    assert (perm_q == perm_r).all(), "one grid, the same keys, a stable sort: the same order twice"
    assert bool((got[0] == torch.arange(1100, device="cuda", dtype=torch.int32)).all()) and bool((got[1] == 0).all())


def test_a_tie_across_reference_blocks_goes_to_the_lowest_row_in_the_last_block(dens):
    Q, R, fe_q, fe_r, (a_q, p, q) = ref.cross_block_tie_sets()
    d2 = block_d2(the_probe(), Q, R)
    got, _, (perm_q, perm_r), _ = check(dens, Q, R, d2, fe_q, fe_r, what="cross-block tie")
    pos = {int(row): k for k, row in enumerate(perm_r)}
    assert pos[p] // 128 == 0 and pos[q] // 128 == 2 and q < p, "the premise, from the device's order: the lower row sits in the last block"
    assert d2[a_q, p] == F32(9.0) and d2[a_q, q] == F32(9.0)
    for k in (0, 2):
        assert int(got[k][a_q]) == q and float(got[k + 1][a_q]) == 9.0, "the least (d2, ROW): a merge on positions would answer p"


def test_the_margin_at_its_sharpest(dens):
    """a reference block whose gap is one ulp below, on, and one ulp above far2_nn: met, not met, not met"""
    tiles = {}
    for which in (-1, 0, 1):
        Q, R, fe_q, fe_r, a_q, gap2 = ref.margin_sets(which)
        d2 = block_d2(the_probe(), Q, R)
        got, info, (perm_q, perm_r), bounds = check(dens, Q, R, d2, fe_q, fe_r, what=("margin", which))
        for b in range(3):
            assert sorted(perm_r[128 * b:128 * (b + 1)].tolist()) == list(range(b, 384, 3)), "the premise: each group fills one block"
        assert bounds == (32, 48) and float(got[1][a_q]) == 9.0 and float(host(got[1]).max()) == 9.0
        assert bool((got[2] == len(R) + 1).all()), "constant free energies: ring 2 is empty"
        tiles[which] = info[0]
    assert tiles == {-1: 48, 0: 32, 1: 32}, "the seed block and M always; the far block only with its gap below far2_nn"


def test_queries_far_from_the_whole_reference_still_have_a_seed(dens):
    Q, R, fe_q, fe_r = ref.far_sets()
    d2 = block_d2(the_probe(), Q, R)
    got, info, _, _ = check(dens, Q, R, d2, fe_q, fe_r, what="far queries")
    assert bool((got[0] != len(R) + 1).all()) and bool((got[1] < FLT_MAX).all()), "every query has a nearest reference"
    assert info[0] >= 16 * cp.n_blocks(len(Q)), "the seed block pairs at least"


@pytest.mark.parametrize("flaw", ["nan query", "inf query", "1e20 query", "nan reference", "inf reference", "1e20 reference",
                                  "nan fe_query", "nan fe_ref"])
def test_flagged_data_is_answered_by_the_direct_kernel(dens, flaw):
    Q0, R0, fq0, fr0, d20 = split_case(300, 1500, 100)
    Q, R, fe_q, fe_r = Q0.copy(), R0.copy(), fq0.copy(), fr0.copy()
    kind, side = flaw.split()
    if side.startswith("fe_"):
        (fe_q if side == "fe_query" else fe_r)[131] = np.nan
        d2 = d20
    else:
        X = Q if side == "query" else R
        X[{"nan": 131, "inf": 40, "1e20": 200}[kind], {"nan": 7, "inf": 99, "1e20": 0}[kind]] = \
            {"nan": np.nan, "inf": np.inf, "1e20": F32(1e20)}[kind]
        assert crossref.stats_flagged(Q, R)
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = block_d2(the_probe(), Q, R)
    q, r, fq, fr = gpu(Q), gpu(R), gpu(fe_q), gpu(fe_r)
    for lo, hi in ((0, 300), (37, 171)):
        got = dens.nearest_reference_wide_pruned(q, r, fq, fr, lo, hi)
        assert dens.wide_against_pruned_info(q.device) == (0, 0, 0)
        direct = dens.nearest_reference(q, r, fq, fr, lo, hi, variant="direct")
        for a, b in zip(got, direct):
            assert (host(a).view(np.uint32) == host(b).view(np.uint32)).all(), "the direct kernel's"
        same_nn(got, expect_nn(d2, fe_q, fe_r, lo, hi), flaw)
    # a NaN outside the query range flags nothing; one in the reference's always does
    if flaw == "nan fe_query":
        check(dens, Q, R, d2, fe_q, fe_r, 140, 300, what="the NaN is outside the range")
    # ... and a clean call behind it in the same workspace runs on the matrix cores again
    check(dens, Q0, R0, d20, fq0, fr0)


def test_a_small_call_behind_a_large_one_and_both_sweeps_alternating_in_one_workspace(dens):
    big, small = split_case(1100, 8320, 80), split_case(33, 129, 100)
    mid = split_case(300, 1500, 100)
    check(dens, big[0], big[1], big[4], big[2], big[3])
    check(dens, small[0], small[1], small[4], small[2], small[3])
    Q, R, fe_q, fe_r, d2 = mid
    radii = cp.radii_for(100, 3)
    q, r = gpu(Q), gpu(R)
    for _ in range(2):
        pops = dens.calculate_populations_against_wide_pruned(q, r, radii, 37, 171)
        assert (host(pops) == crossref.expect_pops(d2, radii, 37, 171)).all()
        perm_q, _ = dens.wide_against_pruned_order(q.device)
        assert sorted(perm_q.tolist()) == list(range(37, 171))
        check(dens, Q, R, d2, fe_q, fe_r)
        perm_q, perm_r = dens.wide_against_pruned_order(q.device)   # the order after a neighbour call: the call's own
        assert sorted(perm_q.tolist()) == list(range(300)) and sorted(perm_r.tolist()) == list(range(1500))
    check(dens, Q, R, d2, fe_q, fe_r, 127, 129)


def test_assign_frames_wide_pruned_with_pruned_neighbours_equals_assign_frames_wide_in_every_entry(dens):
    import torch
    n_q, n_r, D = 200, 600, 100
    Q, R = crossref.sets(D, n_q, n_r, seed=41)
    states_r = (np.arange(n_r) % 5 + 1).astype(np.int32)
    q, r = gpu(Q), gpu(R)
    want = dens.assign_frames_wide(q, r, crossref.radius(D), states_r)
    for pruned_neighbours in (False, True):
        got = dens.assign_frames_wide_pruned(q, r, crossref.radius(D), states_r, pruned_neighbours=pruned_neighbours)
        tiles, mfmas, _ = dens.wide_against_pruned_info(q.device)
        assert 0 < tiles <= 16 * cp.n_blocks(n_q) * cp.n_blocks(n_r) and mfmas == ref.mfmas_per_tile_pair(D) * tiles
        assert set(got) == set(want)
        for key, val in want.items():
            if key == "max_pop":
                assert got[key] == val
            else:
                assert got[key].dtype == val.dtype and got[key].shape == val.shape, key
                assert bool((got[key].view(torch.int32) == val.view(torch.int32)).all()), (key, pruned_neighbours)
    assert int((got["states"] == 0).sum()) == 0


CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from clustering_amd import capi, density as dens
from oracle.oracle import Probe
import crossref, crosswidennpruneref as ref
ORDER = sys.argv[2]
assert capi.lib.dc_hip_canon_order().decode() == ORDER
probe = Probe(ORDER)
cases = [ref.split_case(n_q, n_r, d) for n_q, n_r, d in ((300, 1500, 65), (300, 1500, 100), (129, 33, 256))]
cases.append(ref.cross_block_tie_sets()[:4])
cases.append(ref.margin_sets(-1)[:4])
for Q, R, fe_q, fe_r in cases:
    d2 = crossref.block_d2(probe, Q, R)
    q, r, fq, fr = (crossref.gpu(a) for a in (Q, R, fe_q, fe_r))
    for with_fe in (True, False):
        got = dens.nearest_reference_wide_pruned(q, r, fq if with_fe else None, fr if with_fe else None)
        t, m, e = dens.wide_against_pruned_info(q.device)
        perm_q, perm_r = (p.cpu().numpy().astype(np.int64) for p in dens.wide_against_pruned_order(q.device))
        lo, hi = ref.tile_bounds(Q, R, fe_q if with_fe else None, fe_r if with_fe else None, perm_q, perm_r)
        assert t > 0 and m == ref.mfmas_per_tile_pair(Q.shape[1]) * t and lo <= t <= hi, (Q.shape, R.shape, t, m, lo, hi)
        crossref.same_nn(got, crossref.expect_nn(d2, fe_q if with_fe else None, fe_r if with_fe else None), (Q.shape, R.shape))
        plain = dens.nearest_reference_wide(q, r, fq if with_fe else None, fr if with_fe else None)
        for a, b in zip(got, plain):
            assert (a is None and b is None) or bool((a.view(torch.int32) == b.view(torch.int32)).all()), "the unpruned sweep's"
print("ok")
"""


@pytest.mark.parametrize("order", ["avx", "fma"])
def test_the_libraries_of_the_other_summation_orders(order):
    if not os.path.exists(os.path.join(ROOT, "clustering_amd", "lib_" + order, "libdcdensity.so")):
        pytest.fail(f"clustering_amd/lib_{order}/libdcdensity.so is missing: __graft_entry__.build() makes it")
    env = dict(os.environ, DC_CANON_ORDER=order)
    env.pop("DC_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, order], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
