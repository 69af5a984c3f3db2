"""GPU: the pruned cross population sweep at 257..1024 columns (density.calculate_populations_against_xwide_pruned) against
the referee of tests/test_gpu_cross_wide.py -- the probe's canonical d2 of the [n_q, n_r] block in the library's summation
order (tests/crossref.py) --, bit for bit, and against the unpruned dc_hip_populations_cross_xwide_dev call.  Every finite,
non-empty case asserts the pruning check, a condition on the counters: with the block boxes formed in float64 from the
device's own two orders (xwide_against_pruned_order), every launch evaluates at least the block pairs with gap^2 < r2max and
at most those with gap^2 < 1.001 r2max, 16 tile pairs each, and mfmas == tiles x ceil((2 + 3 D) / 16).  Cases and bounds:
tests/xcrosswidepruneref.py (their premises are checked on the CPU by tests/test_cross_xwide_pruned_cases.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import crossref
import widepruneref as wp
import xcrosswidepruneref as ref
from crossref import block_d2, expect_pops, gpu, host

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
    """(Q, R, d2) of the split stretched blobs: computed once per shape"""
    Q, R = ref.split_sets(n_q, n_r, n_cols)
    return Q, R, block_d2(the_probe(), Q, R)


def same_pops(got, want, what):
    g = host(got)
    if not (g == want).all():
        bad = np.argwhere(g != want)
        k, i = bad[0]
        pytest.fail(f"pops {what}: {len(bad)} entries differ, e.g. radius {k} query {i}: {g[k, i]} != {want[k, i]}")


def run(dens, Q, R, radii, lo=0, hi=None, want=None, bounded=True):
    """one call on finite data with something to sweep -> (populations, (tiles, mfmas, exact), (perm_q, perm_r), (lower,
    upper) of the tile counter, gaps of the block pairs).  Values first -- against want and against the unpruned call --,
    then the counters; bounded=False: a radius below the floor of these widths, whose rule the float64 bounds do not state"""
    q, r = gpu(Q), gpu(R)
    hi = len(Q) if hi is None else hi
    got = dens.calculate_populations_against_xwide_pruned(q, r, radii, lo, hi)
    tiles, mfmas, exact = dens.xwide_against_pruned_info(q.device)
    perm_q, perm_r = (p.cpu().numpy().astype(np.int64) for p in dens.xwide_against_pruned_order(q.device))
    if want is not None:
        same_pops(got, want, (Q.shape, R.shape, radii, lo, hi))
    plain = dens.calculate_populations_against_xwide(q, r, radii, lo, hi)
    assert bool((got == plain).all()), "the unpruned call's populations"
    assert sorted(perm_q.tolist()) == list(range(lo, hi)), "the query order is a permutation of the rows of the range"
    assert sorted(perm_r.tolist()) == list(range(len(R))), "the reference order is a permutation of its rows"
    g = ref.gaps(Q, R, perm_q, perm_r)
    assert g.shape == (ref.query_blocks(lo, hi), ref.n_blocks(len(R))), "the blocks of the gathered range"
    assert mfmas == ref.mfmas_per_tile_pair(Q.shape[1]) * tiles, (tiles, mfmas)
    if not bounded:
        return got, (tiles, mfmas, exact), (perm_q, perm_r), None, g
    lower, upper = ref.tile_bounds(Q, R, perm_q, perm_r, radii)
    print(f"{Q.shape} x {R.shape} [{lo}, {hi}) radii={len(radii)}: tiles {tiles} in [{lower}, {upper}], "
          f"all {16 * g.size * len(wp.launch_r2max(radii))}, exact pairs {exact}")
    if lower > 0:
        assert tiles > 0 and mfmas > 0, "the matrix-core kernel did not answer"
    assert lower <= tiles <= upper, "the pruning check"
    return got, (tiles, mfmas, exact), (perm_q, perm_r), (lower, upper), g


def check(dens, Q, R, d2, radii, lo=0, hi=None):
    got, info, perms, bounds, g = run(dens, Q, R, radii, lo, hi, want=expect_pops(d2, radii, lo, hi))
    return info, perms, bounds, g


POP_SHAPES = [(n_q, n_r, d) for (n_q, n_r), cols in sorted(ref.POP_COLS.items()) for d in cols]


@pytest.mark.parametrize("n_q,n_r,n_cols", POP_SHAPES)
def test_the_split_shapes_prune_to_the_tables_figure(dens, n_q, n_r, n_cols):
    # 300 x 1 500: 3 query blocks against 12; 700 x 2 100: 17 reference blocks in two shares; 1 100 x 8 320: 65 in eight
    Q, R, d2 = split_case(n_q, n_r, n_cols)
    (tiles, _, _), _, (lower, upper), g = check(dens, Q, R, d2, ref.radii_for(n_cols))
    assert wp.shares(g.shape[1]) == {12: 1, 17: 2, 65: 8}[g.shape[1]]
    assert upper < 16 * g.size, "pruning happened"
    if lower == upper:   # (the CPU premise under the numpy order; under the device's order the counter is then pinned)
        assert tiles == 16 * ref.POP_TABLE[(n_q, n_r)][0], (tiles, lower)
    assert int(expect_pops(d2, ref.radii_for(n_cols)).sum()) > 0


@pytest.mark.parametrize("n_cols", ref.COLS)
def test_column_counts(dens, n_cols):
    # every NM mod 4, the ends of the family, both sides of 400 columns
    Q, R, d2 = split_case(300, 1500, n_cols)
    check(dens, Q, R, d2, ref.radii_for(n_cols))


@pytest.mark.parametrize("n_q,n_r", [(1, 300), (127, 300), (128, 300), (129, 300), (1500, 1)])
def test_query_counts_around_a_block_and_a_reference_of_one_row(dens, n_q, n_r):
    Q, R, d2 = split_case(n_q, n_r, 300)
    info, _, _, g = check(dens, Q, R, d2, ref.radii_for(300) + [1e30])
    assert g.shape == ((n_q + 127) // 128, (n_r + 127) // 128)
    assert (expect_pops(d2, [1e30])[0] == n_r).all()


@pytest.mark.parametrize("lo,hi", [(37, 171), (128, 256), (0, 1), (299, 300), (127, 129)])
def test_a_row_range_inside_a_larger_query_array(dens, lo, hi):
    Q, R, d2 = split_case(300, 1500, 300)
    radii = ref.radii_for(300)
    got, info, _, bounds, g = run(dens, Q, R, radii, lo, hi, want=expect_pops(d2, radii, lo, hi))
    outside = np.ones(300, dtype=bool)
    outside[lo:hi] = False
    assert int(host(got)[:, outside].sum()) == 0, "zeros outside the range"
    assert int(host(got)[:, ~outside].sum()) > 0
    assert g.shape[0] == ref.query_blocks(lo, hi) and bounds[1] <= 16 * ref.query_blocks(lo, hi) * 12


@pytest.mark.parametrize("n_cols", [300, 1024])
def test_the_margin_at_its_sharpest(dens, n_cols):
    Q, R, r, (a, b, c, d) = ref.margin_sets(n_cols)
    d2 = block_d2(the_probe(), Q, R)
    info, perms, bounds, g = check(dens, Q, R, d2, [r])
    assert g.shape == (1, 1) and bounds == (16, 16) and info[0] == 16, "the block pair whose box gap is one ulp inside the radius is met"
    assert info[2] > 0, "pairs exactly on a radius can only be decided by the exact path"
    # the pair one ulp inside counts, the pair on the radius and the one an ulp outside do not
    assert d2[a, d] < F32(9.0) and d2[a, b] == F32(9.0) and d2[a, c] > F32(9.0)
    want = expect_pops(d2, [r])
    assert int(want[0][a]) == int((d2[a] < F32(9.0)).sum()) >= 1, "d, and whatever else lies inside; not b, not c"
    eight, eleven = wp.edge_radii(n_cols)
    info8, _, bounds8, _ = check(dens, Q, R, d2, eight)
    info11, _, bounds11, _ = check(dens, Q, R, d2, eleven)
    nm = ref.mfmas_per_tile_pair(n_cols)
    assert bounds8 == (16, 16) and bounds11 == (32, 32), "two launches: the counters add up to the sum of the two bounds"
    assert info8[:2] == (16, 16 * nm) and info11[:2] == (32, 32 * nm)
    want8 = expect_pops(d2, eight)
    assert (want8[eight.index(1e30)] == len(R)).all() and (want8[eight.index(0.0)] == 0).all()


def test_a_positive_radius_below_the_floor_counts_the_duplicates(dens):
    """r = 1e-20: fl32(r^2) is subnormal, below the floor 2^-122 of these widths -- the rule prunes as the floor does, and
    the populations are the numbers of copies"""
    Q, R, copies = ref.duplicate_sets()
    d2 = block_d2(the_probe(), Q, R)
    want = expect_pops(d2, [ref.TINY_RADIUS])
    assert (want[0] == (copies >= 0)).all() and int(want.sum()) == 30, "the referee: one copy each, nothing else"
    got, (tiles, _, _), _, _, g = run(dens, Q, R, [ref.TINY_RADIUS], want=want, bounded=False)
    assert 16 * int((g == 0).sum()) <= tiles <= 16 * int((g < 1.001 * ref.FLOOR).sum()), "the blocks at gap 0, none beyond the floor"
    assert tiles > 0, "the matrix-core kernel answered"
    # ... and beside a radius of ordinary size: the launch prunes by its largest
    radii = [ref.TINY_RADIUS] + ref.radii_for(300)
    check(dens, Q, R, d2, radii)


def test_radius_zero_keeps_no_block(dens):
    Q, R, d2 = split_case(300, 1500, 300)
    info, _, bounds, _ = check(dens, Q, R, d2, [0.0])
    assert bounds == (0, 0) and info == (0, 0, 0), "t = 0 keeps nothing at any floor"


def test_queries_far_from_the_reference_meet_no_block(dens):
    Q, R, _, _ = ref.far_sets()
    d2 = block_d2(the_probe(), Q, R)
    info, _, bounds, _ = check(dens, Q, R, d2, ref.radii_for(300))
    assert bounds == (0, 0) and info[0] == 0
    assert int(expect_pops(d2, ref.radii_for(300)).sum()) == 0


@pytest.mark.parametrize("n_cols", [257, 1024])
def test_nothing_to_prune(dens, n_cols):
    Q, R, radii = ref.unpruned_sets(n_cols)
    d2 = block_d2(the_probe(), Q, R)
    got, info, _, bounds, g = run(dens, Q, R, radii, want=expect_pops(d2, radii))   # (its last call: the unpruned one)
    plain_info = dens.xwide_against_info(got.device)
    assert bounds == (16 * g.size, 16 * g.size) and g.shape == (4, 8)
    print(f"D={n_cols}: exact pairs {info[2]} (unpruned {plain_info[2]})")
    assert info[:2] == plain_info[:2] == (16 * g.size, 16 * g.size * ref.mfmas_per_tile_pair(n_cols))
    # a pair's accumulator depends on the images of its two rows and the chain, not on where the rows stand in an order:
    # with every block pair met, the same pairs go to the exact path
    assert info == plain_info and info[2] > 0, "all three counters are the unpruned call's"


@pytest.mark.parametrize("n_cols", sorted(ref.BAND_PAIRS))
def test_the_exact_path_of_the_1500_by_1500_case_stays_inside_its_cap(dens, n_cols):
    Q, R, d2 = split_case(1500, 1500, n_cols)
    (tiles, mfmas, exact), _, (lower, upper), _ = check(dens, Q, R, d2, ref.radii_for(n_cols))
    count = ref.BAND_PAIRS[n_cols]
    print(f"D={n_cols}: {tiles} tile pairs, {exact} exact pairs = {100.0 * exact / (1024 * tiles):.4f} % of the evaluated pairs, cap {count}")
    assert upper < 16 * 144 and exact <= count <= ref.BAND_SHARE * 1024 * 16 * 64


@pytest.mark.parametrize("n_cols", [300, 512])   # (beyond 400 columns the column-chunked direct kernel answers)
@pytest.mark.parametrize("flaw", ["nan query", "inf reference", "1e20 query"])
def test_flagged_data_is_answered_by_the_direct_kernel(dens, flaw, n_cols):
    Q0, R0, d20 = split_case(300, 1500, n_cols)
    Q, R = Q0.copy(), R0.copy()
    kind, side = flaw.split()
    X = Q if side == "query" else R
    X[{"nan": 131, "inf": 40, "1e20": 200}[kind], {"nan": 7, "inf": n_cols - 1, "1e20": 0}[kind]] = \
        {"nan": np.nan, "inf": np.inf, "1e20": F32(1e20)}[kind]
    assert crossref.stats_flagged(Q, R)
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = block_d2(the_probe(), Q, R)
    radii = ref.radii_for(n_cols)
    q, r = gpu(Q), gpu(R)
    for lo, hi in ((0, 300), (37, 171)):
        got = dens.calculate_populations_against_xwide_pruned(q, r, radii, lo, hi)
        assert dens.xwide_against_pruned_info(q.device) == (0, 0, 0)
        assert bool((got == dens.calculate_populations_against_xwide(q, r, radii, lo, hi)).all()), "the unpruned call's"
        assert dens.xwide_against_info(q.device) == (0, 0, 0), "there too the direct kernel answered"
        same_pops(got, expect_pops(d2, radii, lo, hi), flaw)
    # ... and a clean call behind it in the same workspace runs on the matrix cores again
    info, _, _, _ = check(dens, Q0, R0, d20, radii)
    assert info[0] > 0


def test_a_small_call_behind_a_large_one_in_the_same_workspace(dens):
    check(dens, *split_case(1100, 8320, 257), ref.radii_for(257))
    check(dens, *split_case(1, 300, 300), ref.radii_for(300))
    check(dens, *split_case(300, 1500, 1024), ref.radii_for(1024))
    Q, R, d2 = split_case(300, 1500, 300)
    check(dens, Q, R, d2, ref.radii_for(300), 37, 171)


def test_the_order_reader_refuses_other_shapes_a_self_order_and_the_other_family(dens):
    import torch
    from clustering_amd import capi
    Q, R, d2 = split_case(300, 1500, 300)
    check(dens, Q, R, d2, ref.radii_for(300), 37, 171)
    dev = torch.device("cuda", torch.cuda.current_device())
    ws = dens._cached("xwide_against_pruned", dev).buf
    perm_q = torch.empty(1500, dtype=torch.int32, device="cuda")
    perm_r = torch.empty(1500, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    cross, self_order = capi.lib.dc_hip_cross_xwide_pruned_order_dev, capi.lib.dc_hip_xwide_pruned_order_dev
    assert cross(p(ws), 134, 1500, 300, p(perm_q), p(perm_r), None) == 0
    assert sorted(perm_q[:134].tolist()) == list(range(37, 171))
    for shape in ((133, 1500, 300), (300, 1500, 300), (134, 1499, 300), (134, 1500, 301), (1500, 134, 300)):
        assert cross(p(ws), *shape, p(perm_q), p(perm_r), None) == -1, shape
    blank = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    assert cross(p(blank), 134, 1500, 300, p(perm_q), p(perm_r), None) == -1
    # the cross workspace holds no self order of either of its sets ...
    assert self_order(p(ws), 1500, 300, p(perm_r), None) == -1 and self_order(p(ws), 134, 300, p(perm_q), None) == -1
    # ... the workspace of a pruned self sweep of these widths holds no cross order, whatever the shape asked for ...
    c = gpu(R)
    dens.calculate_populations_xwide_pruned(c, ref.radii_for(300))
    ws_self = dens._cached("xwide_pruned", dev).buf
    assert self_order(p(ws_self), 1500, 300, p(perm_r), None) == 0
    for n_q in (1500, 134):
        assert cross(p(ws_self), n_q, 1500, 300, p(perm_r), p(perm_r), None) == -1
    # ... and neither does a workspace of the 65..256 family: its reader refuses these widths, this one those
    Qw, Rw = Q[:, :200].copy(), R[:, :200].copy()
    dens.calculate_populations_against_wide_pruned(gpu(Qw), gpu(Rw), ref.radii_for(300))
    ws_wide = dens._wide_against_pruned_workspace(dev).buf
    wide_cross = capi.lib.dc_hip_cross_wide_pruned_order_dev
    assert wide_cross(p(ws_wide), 300, 1500, 200, p(perm_q), p(perm_r), None) == 0
    assert cross(p(ws_wide), 300, 1500, 200, p(perm_q), p(perm_r), None) == -1, "200 columns: not this family's"
    assert cross(p(ws_wide), 300, 1500, 300, p(perm_q), p(perm_r), None) == -1, "the order it holds is of 200 columns"
    assert wide_cross(p(ws), 134, 1500, 300, p(perm_q), p(perm_r), None) == -1
    z256, z257 = torch.zeros((10, 256), device="cuda"), torch.zeros((10, 257), device="cuda")
    with pytest.raises(ValueError, match="257..1024"):
        dens.calculate_populations_against_xwide_pruned(z256, z256, [1.0])
    with pytest.raises(ValueError, match="65..256"):
        dens.calculate_populations_against_wide_pruned(z257, z257, [1.0])


def test_every_counter_reader_answers_from_the_workspace_of_its_own_kind(dens):
    import torch
    Q, R, d2 = split_case(300, 1500, 300)
    q, r = gpu(Q), gpu(R)
    radii = ref.radii_for(300)
    dens.calculate_populations_against_xwide(q, r, radii)
    plain = dens.xwide_against_info(q.device)
    info, _, _, _ = check(dens, Q, R, d2, radii)
    assert plain[0] == 16 * 3 * 12 > info[0] > 0
    got = dens.calculate_populations_against_xwide_pruned(q, r, radii, 5, 5)
    assert int(got.abs().sum()) == 0 and dens.xwide_against_pruned_info(q.device) == (0, 0, 0)
    assert dens.xwide_against_info(q.device) == plain, "an empty pruned call leaves the unpruned kind's counters alone"
