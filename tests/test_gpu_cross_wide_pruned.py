"""GPU: the pruned wide cross population sweep (density.calculate_populations_against_wide_pruned, 65..256 columns)
against the probe's canonical d2 of the [n_q, n_r] block (tests/crossref.py), bit for bit.  Every finite, non-empty case
first asserts that the matrix-core kernel answered (wide_against_pruned_info: nm_for(D) MFMAs per tile pair, and tile
pairs > 0 wherever the lower bound is) and then the pruning check, a condition on the counter: with the block boxes formed
in float64 from the device's own two orders (wide_against_pruned_order), every launch evaluates at least the block pairs
with gap^2 < r2max and at most those with gap^2 < 1.001 r2max, 16 tile pairs each.  Cases and bounds:
tests/crosswidepruneref.py (their premises are checked on the CPU by tests/test_cross_wide_pruned_cases.py)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import crossref
import crosswidepruneref as ref
import crosswideref as cw
import widepruneref as wp
from crossref import block_d2, expect_pops, gpu, host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    """(Q, R, d2) of the split stretched blobs: computed once per shape"""
    Q, R = ref.split_sets(n_q, n_r, n_cols)
    return Q, R, block_d2(the_probe(), Q, R)


def std_radii(n_cols):
    return ref.radii_for(n_cols, 3)


def same_pops(got, want, what):
    g = host(got)
    if not (g == want).all():
        bad = np.argwhere(g != want)
        k, i = bad[0]
        pytest.fail(f"pops {what}: {len(bad)} entries differ, e.g. radius {k} query {i}: {g[k, i]} != {want[k, i]}")


def run(dens, Q, R, radii, lo=0, hi=None, q=None, r=None):
    """one call on finite data with something to sweep -> (populations, (tiles, mfmas, exact), (perm_q, perm_r), (lower,
    upper) of the tile counter, gaps of the block pairs); asserts the counters"""
    q = gpu(Q) if q is None else q
    r = gpu(R) if r is None else r
    hi = len(Q) if hi is None else hi
    got = dens.calculate_populations_against_wide_pruned(q, r, radii, lo, hi)
    tiles, mfmas, exact = dens.wide_against_pruned_info(q.device)
    perm_q, perm_r = (p.cpu().numpy().astype(np.int64) for p in dens.wide_against_pruned_order(q.device))
    assert sorted(perm_q.tolist()) == list(range(lo, hi)), "the query order is a permutation of the rows of the range"
    assert sorted(perm_r.tolist()) == list(range(len(R))), "the reference order is a permutation of its rows"
    g = ref.gaps(Q, R, perm_q, perm_r)
    assert g.shape == (ref.query_blocks(lo, hi), ref.n_blocks(len(R))), "the blocks of the gathered range"
    lower, upper = ref.tile_bounds(Q, R, perm_q, perm_r, radii)
    print(f"{Q.shape} x {R.shape} [{lo}, {hi}) radii={len(radii)}: tiles {tiles} in [{lower}, {upper}], "
          f"all {16 * g.size * len(ref.launch_r2max(radii))}, exact pairs {exact}")
    if lower > 0:
        assert tiles > 0 and mfmas > 0, "the matrix-core kernel did not answer"
    assert mfmas == cw.nm_for(Q.shape[1]) * tiles, (tiles, mfmas)
    assert lower <= tiles <= upper, "the pruning check"
    return got, (tiles, mfmas, exact), (perm_q, perm_r), (lower, upper), g


def check(dens, Q, R, d2, radii, lo=0, hi=None, what=""):
    got, info, perms, bounds, g = run(dens, Q, R, radii, lo, hi)
    same_pops(got, expect_pops(d2, radii, lo, hi), (what, Q.shape, R.shape, radii, lo, hi))
    return info, perms, bounds, g


@pytest.mark.parametrize("n_cols", [65, 84, 85, 128, 256])
def test_column_counts(dens, n_cols):
    Q, R, d2 = split_case(300, 300, n_cols)
    check(dens, Q, R, d2, std_radii(n_cols))


@pytest.mark.parametrize("n_q,n_r,n_cols", [(1, 300, 100), (300, 1, 100), (33, 129, 100), (129, 33, 100), (300, 1500, 100),
                                            (1500, 300, 100), (700, 2100, 100), (1100, 8320, 80)])
def test_rectangles_in_both_orientations_and_every_padding(dens, n_q, n_r, n_cols):
    # 300 x 1 500: 3 query blocks against 12 reference blocks -- and 1 500 x 300: 12 against 3, more query blocks than the
    # reference has blocks at all; 700 x 2 100: 17 reference blocks in two shares; 1 100 x 8 320: 65 in eight
    Q, R, d2 = split_case(n_q, n_r, n_cols)
    info, perms, (lower, upper), g = check(dens, Q, R, d2, std_radii(n_cols))
    assert wp.shares(g.shape[1]) == {1: 1, 2: 1, 3: 1, 12: 1, 17: 2, 65: 8}[g.shape[1]]
    if (n_q, n_r, n_cols) in ref.SPLIT_TABLE:
        assert upper < 16 * g.size, "pruning happened"
    assert int(expect_pops(d2, std_radii(n_cols)).sum()) > 0


@pytest.mark.parametrize("lo,hi", [(37, 171), (128, 256), (0, 1), (299, 300), (100, 300), (127, 129)])
def test_row_ranges_that_start_and_end_inside_tiles_and_blocks(dens, lo, hi):
    Q, R, d2 = split_case(300, 1500, 100)
    got, info, (perm_q, perm_r), bounds, g = run(dens, Q, R, std_radii(100), lo, hi)
    want = expect_pops(d2, std_radii(100), lo, hi)
    same_pops(got, want, ("range", lo, hi))
    outside = np.ones(300, dtype=bool)
    outside[lo:hi] = False
    assert int(host(got)[:, outside].sum()) == 0 and int(want[:, outside].sum()) == 0, "zeros outside the range"
    assert g.shape[0] == ref.query_blocks(lo, hi) and bounds[1] <= 16 * ref.query_blocks(lo, hi) * 12


def test_an_empty_side_and_an_empty_range_give_zeros_and_sweep_nothing(dens):
    import torch
    Q0, R0, d20 = split_case(33, 129, 100)
    for n_q, n_r in ((40, 0), (0, 40), (0, 0)):
        check(dens, Q0, R0, d20, std_radii(100))   # (a call before it leaves counters behind that the empty call must not keep)
        q = torch.zeros((n_q, 100), dtype=torch.float32, device="cuda")
        r = torch.zeros((n_r, 100), dtype=torch.float32, device="cuda")
        got = dens.calculate_populations_against_wide_pruned(q, r, [0.5, 1e30])
        assert got.shape == (2, n_q) and int(got.abs().sum()) == 0
        assert dens.wide_against_pruned_info(q.device) == (0, 0, 0)
    check(dens, Q0, R0, d20, std_radii(100))
    got = dens.calculate_populations_against_wide_pruned(gpu(Q0), gpu(R0), std_radii(100), 5, 5)
    assert got.shape == (3, 33) and int(got.abs().sum()) == 0
    assert dens.wide_against_pruned_info(got.device) == (0, 0, 0)
    from clustering_amd.capi import DensityLibraryError
    with pytest.raises(DensityLibraryError):
        dens.wide_against_pruned_order(got.device)   # nothing swept: the workspace holds no order


def test_radius_zero_keeps_no_block(dens):
    Q, R, d2 = split_case(300, 1500, 100)
    info, _, bounds, _ = check(dens, Q, R, d2, [0.0])
    assert bounds == (0, 0) and info == (0, 0, 0), "t = 0 keeps nothing"
    assert int(expect_pops(d2, [0.0]).sum()) == 0, "no self term: every count is 0"


def test_queries_far_from_the_reference_meet_no_block(dens):
    Q, R, _ = split_case(300, 1500, 100)
    Q = Q.copy()
    Q[:, 0] += np.float32(100.0)
    d2 = block_d2(the_probe(), Q, R)
    info, _, bounds, _ = check(dens, Q, R, d2, std_radii(100))
    assert bounds == (0, 0) and info[0] == 0
    assert int(expect_pops(d2, std_radii(100)).sum()) == 0


def test_units_without_a_survivor_beside_units_with_one(dens):
    Q, R = ref.mixed_units_sets()
    d2 = block_d2(the_probe(), Q, R)
    radii = [ref.MIXED_RADIUS]
    info, perms, (lower, upper), g = check(dens, Q, R, d2, radii)
    empty, units = ref.empty_units(g, ref.launch_r2max(radii)[0])
    print(f"{empty} of {units} (query block, share) units without a survivor")
    assert units == 9 * 8 and 0 < empty < units, "the premise, from the device's orders: both kinds of unit"
    assert 0 < lower and upper < 16 * g.size


def test_nothing_to_prune(dens):
    radii = std_radii(100) + [1e30]
    Q, R, d2 = split_case(700, 2100, 100)
    q, r = gpu(Q), gpu(R)
    got, info, _, bounds, g = run(dens, Q, R, radii, q=q, r=r)
    want = expect_pops(d2, radii)
    same_pops(got, want, "1e30")
    plain = dens.calculate_populations_against_wide(q, r, radii)
    assert info[0] == 16 * g.shape[0] * g.shape[1] == 16 * 6 * 17 == dens.wide_against_info(q.device)[0]
    same_pops(plain, want, "unpruned")
    assert (want[3] == len(R)).all()


def test_the_margin_at_its_sharpest(dens):
    Q, R, r, (a, b, c, d) = ref.margin_sets()
    d2 = block_d2(the_probe(), Q, R)
    info, perms, bounds, g = check(dens, Q, R, d2, [r])
    assert g.shape == (1, 1) and bounds == (16, 16) and info[0] == 16, "the block pair whose box gap is one ulp inside the radius is met"
    assert info[2] > 0, "pairs exactly on a radius can only be decided by the exact path"
    # the pair one ulp inside counts, the pair on the radius and the one an ulp outside do not
    assert d2[a, d] < np.float32(9.0) and d2[a, b] == np.float32(9.0) and d2[a, c] > np.float32(9.0)
    want = expect_pops(d2, [r])
    assert int(want[0][a]) == int((d2[a] < np.float32(9.0)).sum()) >= 1, "d, and whatever else lies inside; not b, not c"
    eight, eleven = wp.edge_radii()
    info8, _, bounds8, _ = check(dens, Q, R, d2, eight)
    info11, _, bounds11, _ = check(dens, Q, R, d2, eleven)
    assert bounds8 == (16, 16) and bounds11 == (32, 32), "two launches: the counters add up to the sum of the two bounds"
    assert info8[:2] == (16, 16 * 16) and info11[:2] == (32, 32 * 16)
    want8 = expect_pops(d2, eight)
    assert (want8[eight.index(1e30)] == len(R)).all() and (want8[eight.index(0.0)] == 0).all()


def test_pairs_on_a_radius_across_the_sets(dens):
    Q, R, r_edge, groups = cw.boundary_sets(300, 300, 80)
    d2 = block_d2(the_probe(), Q, R)
    base = float(np.sqrt(2 * 0.3 * 0.3 * 80))
    for radii in ([r_edge], [base * 1.1, r_edge, base * 0.9]):
        info, _, _, _ = check(dens, Q, R, d2, radii, what="boundary")
        assert info[2] > 0
        want = expect_pops(d2, radii)
        for a, b, c, d in groups:
            assert want[radii.index(r_edge)][a] >= 1   # (the pair one ulp inside the radius counts, the one on it does not)


def test_queries_and_reference_in_the_same_array(dens):
    """Q == R, the same tensor: an ordinary pair of sets -- every row counts itself"""
    import torch
    c = wp.stretched(1100, 100)
    d2 = block_d2(the_probe(), c, c)
    ct = torch.from_numpy(c).cuda()
    radii = std_radii(100)
    got, info, (perm_q, perm_r), _, _ = run(dens, c, c, radii, q=ct, r=ct)
    same_pops(got, expect_pops(d2, radii), "Q == R")
    assert (perm_q == perm_r).all(), "one grid, the same keys, a stable sort: the same order twice"
    assert bool((got == dens.calculate_populations_wide(ct, radii)).all()), "for r > 0 the pair (i, i) is the self sweep's own 1"
    assert (expect_pops(d2, radii) >= 1).all()


def test_duplicates_between_and_within_the_sets(dens):
    Q, R = crossref.sets(100, 300, 700, seed=19)
    d2 = block_d2(the_probe(), Q, R)
    assert int((d2 == 0).sum()) > 0
    check(dens, Q, R, d2, [crossref.radius(100), 1e-3, 0.0], what="duplicates")


@pytest.mark.parametrize("flaw", ["nan query", "inf query", "1e20 query", "nan reference", "inf reference", "1e20 reference"])
def test_flagged_data_is_answered_by_the_direct_kernel(dens, flaw):
    Q0, R0, d20 = split_case(300, 300, 100)
    Q, R = Q0.copy(), R0.copy()
    kind, side = flaw.split()
    X = Q if side == "query" else R
    X[{"nan": 131, "inf": 40, "1e20": 200}[kind], {"nan": 7, "inf": 99, "1e20": 0}[kind]] = \
        {"nan": np.nan, "inf": np.inf, "1e20": np.float32(1e20)}[kind]
    assert crossref.stats_flagged(Q, R)
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = block_d2(the_probe(), Q, R)
    radii = std_radii(100)
    q, r = gpu(Q), gpu(R)
    for lo, hi in ((0, 300), (37, 171)):
        got = dens.calculate_populations_against_wide_pruned(q, r, radii, lo, hi)
        assert dens.wide_against_pruned_info(q.device) == (0, 0, 0)
        assert bool((got == dens.calculate_populations_against(q, r, radii, lo, hi, variant="direct")).all()), "the direct kernel's"
        same_pops(got, expect_pops(d2, radii, lo, hi), flaw)
    # ... and a clean call behind it in the same workspace runs on the matrix cores again
    info, _, bounds, _ = check(dens, Q0, R0, d20, radii)
    assert info[0] > 0


def test_a_small_call_behind_a_large_one_in_the_same_workspace(dens):
    check(dens, *split_case(1100, 8320, 80), std_radii(80))
    check(dens, *split_case(33, 129, 100), std_radii(100))
    check(dens, *split_case(300, 300, 256), std_radii(256))
    Q, R, d2 = split_case(300, 1500, 100)
    check(dens, Q, R, d2, std_radii(100), 37, 171)


def test_the_order_of_another_shape_is_refused_and_a_self_order_is_no_cross_order(dens):
    import torch
    from clustering_amd import capi
    Q, R, d2 = split_case(300, 1500, 100)
    check(dens, Q, R, d2, std_radii(100), 37, 171)
    dev = torch.device("cuda", torch.cuda.current_device())
    ws = dens._wide_against_pruned_workspace(dev).buf
    perm_q = torch.empty(300, dtype=torch.int32, device="cuda")
    perm_r = torch.empty(1500, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    cross, self_order = capi.lib.dc_hip_cross_wide_pruned_order_dev, capi.lib.dc_hip_wide_pruned_order_dev
    assert cross(p(ws), 134, 1500, 100, p(perm_q), p(perm_r), None) == 0
    assert sorted(perm_q[:134].tolist()) == list(range(37, 171))
    for shape in ((133, 1500, 100), (300, 1500, 100), (134, 1499, 100), (134, 1500, 101), (1500, 134, 100)):
        assert cross(p(ws), *shape, p(perm_q), p(perm_r), None) == -1, shape
    blank = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    assert cross(p(blank), 134, 1500, 100, p(perm_q), p(perm_r), None) == -1
    # the cross workspace holds no self order of either of its sets
    assert self_order(p(ws), 1500, 100, p(perm_r), None) == -1 and self_order(p(ws), 134, 100, p(perm_q), None) == -1
    # ... and the workspace of a pruned self sweep holds no cross order, whatever the shape asked for
    c = torch.from_numpy(np.ascontiguousarray(R)).cuda()
    dens.calculate_populations_wide_pruned(c, std_radii(100))
    ws_self = dens._wide_pruned_workspace(dev).buf
    assert self_order(p(ws_self), 1500, 100, p(perm_r), None) == 0
    for n_q in (1500, 134):
        assert cross(p(ws_self), n_q, 1500, 100, p(perm_r), p(perm_r), None) == -1


def test_assign_frames_wide_pruned_equals_assign_frames_wide_in_every_entry(dens):
    import torch
    n_q, n_r, D = 200, 600, 100
    Q, R = crossref.sets(D, n_q, n_r, seed=41)
    states_r = (np.arange(n_r) % 5 + 1).astype(np.int32)
    q, r = gpu(Q), gpu(R)
    want = dens.assign_frames_wide(q, r, crossref.radius(D), states_r)
    got = dens.assign_frames_wide_pruned(q, r, crossref.radius(D), states_r)
    tiles, mfmas, _ = dens.wide_against_pruned_info(q.device)
    assert 0 < tiles <= cw.tile_pairs(n_q, n_r) and mfmas == cw.nm_for(D) * tiles, "the pruned sweep answered"
    assert set(got) == set(want)
    for key, val in want.items():
        if key == "max_pop":
            assert got[key] == val
        else:
            assert got[key].dtype == val.dtype and got[key].shape == val.shape, key
            assert bool((got[key].view(torch.int32) == val.view(torch.int32)).all()), key
    assert int((got["states"] == 0).sum()) == 0


CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from clustering_amd import capi, density as dens
from oracle.oracle import Probe
import crossref, crosswideref as cw, crosswidepruneref as ref
ORDER = sys.argv[2]
assert capi.lib.dc_hip_canon_order().decode() == ORDER
probe = Probe(ORDER)
cases = [(ref.split_sets(n_q, n_r, d), ref.radii_for(d, 3)) for n_q, n_r, d in ((300, 300, 65), (300, 1500, 100), (129, 33, 256))]
cases.append((cw.boundary_sets(300, 300, 80)[:2], [cw.BOUNDARY_RADIUS, float(np.sqrt(0.18 * 80))]))
Qm, Rm, r, _ = ref.margin_sets()
cases.append(((Qm, Rm), [r]))
for (Q, R), radii in cases:
    d2 = crossref.block_d2(probe, Q, R)
    q, rr = crossref.gpu(Q), crossref.gpu(R)
    got = dens.calculate_populations_against_wide_pruned(q, rr, radii)
    t, m, e = dens.wide_against_pruned_info(q.device)
    perm_q, perm_r = (p.cpu().numpy().astype(np.int64) for p in dens.wide_against_pruned_order(q.device))
    lo, hi = ref.tile_bounds(Q, R, perm_q, perm_r, radii)
    assert t > 0 and m == cw.nm_for(Q.shape[1]) * t and lo <= t <= hi, (Q.shape, R.shape, t, m, lo, hi)
    assert (crossref.host(got) == crossref.expect_pops(d2, radii)).all(), (Q.shape, R.shape, "pops")
    plain = dens.calculate_populations_against_wide(q, rr, radii)
    assert bool((got == plain).all()), (Q.shape, R.shape, "the unpruned sweep's")
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


@pytest.mark.parametrize("n_cols", [65, 256])
def test_at_most_one_percent_of_the_evaluated_pairs_go_to_the_exact_path(dens, n_cols):
    Q, R, d2 = split_case(1500, 1500, n_cols)
    (tiles, mfmas, exact), _, _, _ = check(dens, Q, R, d2, std_radii(n_cols))
    print(f"D={n_cols}: {tiles} tile pairs, {exact} exact pairs = {100.0 * exact / (1024 * tiles):.4f} % of the evaluated pairs")
    assert exact <= 0.01 * 1024 * tiles


def test_every_counter_and_order_reader_answers_from_the_workspace_of_its_own_kind(dens):
    """The four wide kinds keep a cached workspace each: a call of one kind must show in that kind's reader alone.  300 rows
    (three blocks of 128, the last one partial: the smallest shape with more than one block) and 200 queries against them,
    65 columns.  A call that sweeps nothing -- an empty row range; for the pruned self sweep segment 3 of 4, which owns no
    block of three -- turns its own reader to (0, 0, 0) and leaves the other three as they were."""
    import torch
    n_q, n_r, D = 200, 300, 65
    Q, R = crossref.sets(D, n_q, n_r, seed=43)
    q, r = gpu(Q), gpu(R)
    radii = [crossref.radius(D)]
    dev = torch.device("cuda", torch.cuda.current_device())
    readers = {"wide": dens.wide_sweep_info, "wide pruned": dens.wide_pruned_info, "against wide": dens.wide_against_info,
               "against wide pruned": dens.wide_against_pruned_info}
    sweeps = {"wide": lambda *span: dens.calculate_populations_wide(r, radii, *span),
              "wide pruned": lambda *span: dens.calculate_populations_wide_pruned(r, radii, *span),
              "against wide": lambda *span: dens.calculate_populations_against_wide(q, r, radii, *span),
              "against wide pruned": lambda *span: dens.calculate_populations_against_wide_pruned(q, r, radii, *span)}
    nothing = {"wide": (0, 0), "wide pruned": (3, 4), "against wide": (0, 0), "against wide pruned": (0, 0)}
    for kind, sweep in sweeps.items():
        sweep()
    state = {kind: read(dev) for kind, read in readers.items()}
    print(state)
    for kind, (tiles, mfmas, _) in state.items():
        assert tiles > 0 and mfmas == cw.nm_for(D) * tiles, (kind, "the matrix-core sweep answered")
    perm = dens.wide_pruned_order(dev)
    perm_q, perm_r = dens.wide_against_pruned_order(dev)
    assert sorted(perm.tolist()) == list(range(n_r)), "the self order: a permutation of the 300 rows"
    assert sorted(perm_q.tolist()) == list(range(n_q)) and sorted(perm_r.tolist()) == list(range(n_r)), "the cross orders: 200 and 300"
    for kind, sweep in sweeps.items():
        got = sweep(*nothing[kind])
        assert int(got.abs().sum()) == 0, (kind, "nothing swept, nothing counted")
        state[kind] = (0, 0, 0)
        assert {k: read(dev) for k, read in readers.items()} == state, f"after the empty {kind} call"
