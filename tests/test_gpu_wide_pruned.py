"""GPU: the pruned wide population sweep (density.calculate_populations_wide_pruned, 65..256 columns) against the CPU
oracle, bit for bit.  Every finite case first asserts that the matrix-core kernel answered (wide_pruned_info: tiles > 0)
and then the pruning check, a condition on the counter: with the block boxes formed in float64 from the device's own order
(wide_pruned_order), every launch evaluates at least the block pairs with gap^2 < r2max and at most those with
gap^2 < 1.001 r2max, 16 tile pairs each.  Cases and bounds: tests/widepruneref.py (their premises are checked on the CPU
by tests/test_wide_pruned_cases.py)."""
import functools

import numpy as np
import pytest

import wideref
import widepruneref as ref

pytestmark = pytest.mark.gpu
TABLE = ref.STRETCHED_TABLE


@pytest.fixture(scope="module")
def dens():
    import torch
    assert torch.cuda.is_available()
    from clustering_amd import density
    return density


def u64(t):
    return t.cpu().numpy().astype(np.uint32).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def reference(n_rows, n_cols, radii):
    """(coords, populations) of the stretched blobs: computed once per shape and list of radii"""
    from oracle.oracle import Oracle
    c = ref.stretched(n_rows, n_cols)
    return c, Oracle().populations(c, list(radii))


def std_radii(n_cols):
    return tuple(ref.radii_for(n_cols, 3))


def run(dens, c, radii, segment=0, n_segments=0, finite=True):
    """one call -> (populations as uint64, (tiles, mfmas, exact), order, (lower, upper) of the tile counter)"""
    import torch
    ct = torch.from_numpy(c).cuda()
    got = dens.calculate_populations_wide_pruned(ct, list(radii), segment, n_segments)
    info = dens.wide_pruned_info(ct.device)
    perm = dens.wide_pruned_order(ct.device).cpu().numpy().astype(np.int64)
    assert sorted(perm.tolist()) == list(range(len(c))), "the order is a permutation of the rows"
    if not finite:
        return u64(got), info, perm, None
    lo, hi = ref.tile_bounds(c, perm, list(radii), segment, n_segments)
    print(f"{c.shape} radii={len(radii)} segment {segment}/{n_segments}: tiles {info[0]} in [{lo}, {hi}], "
          f"all {16 * ref.n_blocks(len(c)) ** 2 * len(ref.launch_r2max(list(radii)))}, exact pairs {info[2]}")
    if lo > 0:
        assert info[0] > 0 and info[1] > 0, "the matrix-core kernel did not answer"
    assert lo <= info[0] <= hi, "the pruning check"
    assert info[1] == info[0] * mfmas_per_tile_pair(c.shape[1])
    return u64(got), info, perm, (lo, hi)


def mfmas_per_tile_pair(n_cols):
    return (2 + 3 * n_cols + 15) // 16   # two constant slots and three products per column, 16 K slots per MFMA


def check(dens, c, radii, want):
    got, info, perm, bounds = run(dens, c, radii)
    assert (got == want).all(), ("populations", c.shape, radii)
    return info, perm, bounds


@pytest.mark.parametrize("n_cols", [65, 84, 85, 128, 256])
def test_column_counts(dens, n_cols):
    c, want = reference(300, n_cols, std_radii(n_cols))
    check(dens, c, std_radii(n_cols), want)


@pytest.mark.parametrize("n_rows,n_cols", [(1, 100), (31, 100), (33, 100), (129, 100), (700, 100), (1500, 100), (2100, 100),
                                           (8320, 80)])
def test_row_counts_from_one_frame_to_a_second_launch_group(dens, n_rows, n_cols):
    radii = std_radii(n_cols)
    c, want = reference(n_rows, n_cols, radii + (1e-3, 0.0))
    info, perm, (lo, hi) = check(dens, c, radii, want[:3])
    if (n_rows, n_cols) in TABLE:
        assert hi < 16 * ref.n_blocks(n_rows) ** 2, "pruning happened"
    if n_rows == 1:
        assert int(want[0][0]) == 1 and info[0] == 16


def test_shares_without_a_survivor(dens):
    # 8 320 rows: 65 blocks in 8 shares; at these radii a query block meets the blocks whose boxes touch its own, so
    # (query block, share) units are left without a survivor -- they run no chain and still add the frames' own 1 (share 0)
    c, want = reference(8320, 80, std_radii(80) + (1e-3, 0.0))
    radii = [1e-3, 0.0]
    info, perm, (lo, hi) = check(dens, c, radii, want[3:])
    nb = ref.n_blocks(len(c))
    assert info[0] >= 16 * nb
    empty, units = ref.empty_units(c, perm, ref.launch_r2max(radii)[0])
    print(f"{empty} of {units} (query block, share) units without a survivor")
    assert units == 8 * nb and empty > 0, "the premise, from the device's order: there are such units"
    assert (want[3:] >= 1).all() and (want[4] == 1).all()


def test_the_margin_at_its_sharpest(dens, oracle):
    c, r, (a, b, cc, d) = ref.margin_case()
    want = oracle.populations(c, [r])
    info, perm, bounds = check(dens, c, [r], want)
    assert sorted(perm[:128].tolist()) == list(range(0, 256, 2)) and sorted(perm[128:].tolist()) == list(range(1, 256, 2)), \
        "each group fills one block"
    assert bounds == (64, 64) and info[0] == 64, "the block pair whose box gap is one ulp inside the radius is met"
    assert info[2] > 0, "pairs exactly on a radius can only be decided by the exact path"
    # the pair one ulp inside counts, the pair on the radius and the one an ulp outside do not
    x = c.astype(np.float64)
    d2 = ((x[a][None, :] - x) ** 2).sum(axis=1)
    assert d2[d] < 9.0 and d2[b] == 9.0 and d2[cc] > 9.0
    assert int(want[0][a]) == int((d2 < 9.0).sum()), "a itself, d, and whatever else lies inside; not b, not c"
    eight, eleven = ref.edge_radii()
    want8 = oracle.populations(c, eight)
    info8, _, bounds8 = check(dens, c, eight, want8)
    info11, _, bounds11 = check(dens, c, eleven, oracle.populations(c, eleven))
    assert bounds8 == (64, 64) and bounds11 == (128, 128), "two launches: the counters add up to the sum of the two bounds"
    assert info8[:2] == (64, 64 * 16) and info11[:2] == (128, 128 * 16)
    assert (want8[eight.index(1e30)] == len(c)).all() and (want8[eight.index(0.0)] == 1).all()


def test_nothing_to_prune(dens):
    import torch
    radii = std_radii(100) + (1e30,)
    c, want = reference(700, 100, radii)
    info, perm, bounds = check(dens, c, radii, want)
    nb = ref.n_blocks(len(c))
    ct = torch.from_numpy(c).cuda()
    plain = dens.calculate_populations_wide(ct, list(radii))
    assert info[0] == 16 * nb * nb == dens.wide_sweep_info(ct.device)[0]
    assert (u64(plain) == want).all() and (want[3] == len(c)).all()


@pytest.mark.parametrize("n_segments", [2, 3, 5, 40])
def test_segments_of_the_order(dens, n_segments):
    radii = std_radii(100)
    c, want = reference(1500, 100, radii + (1e-3, 0.0))
    want = want[:3]
    _, whole, _, _ = run(dens, c, radii)
    total = np.zeros_like(want)
    tiles = mfmas = 0
    for seg in range(n_segments):
        got, info, perm, bounds = run(dens, c, radii, seg, n_segments)
        blocks = list(ref.segment_blocks(len(c), seg, n_segments))
        rows = np.concatenate([perm[128 * b:128 * (b + 1)] for b in blocks]) if blocks else np.zeros(0, dtype=np.int64)
        mine = np.zeros(len(c), dtype=bool)
        mine[rows] = True
        assert (got[:, ~mine] == 0).all(), "zero outside the rows of its blocks"
        assert (got[:, mine] == want[:, mine]).all(), "the final counts of its rows"
        if not blocks:
            assert info == (0, 0, 0) and bounds == (0, 0)
        total += got
        tiles += info[0]
        mfmas += info[1]
    assert (total == want).all()
    assert (tiles, mfmas) == whole[:2], "the tile counts add up to those of the whole call"


def test_no_segments_is_the_whole_sweep_whatever_the_segment_argument_holds(dens):
    radii = std_radii(100)
    c, want = reference(1500, 100, radii + (1e-3, 0.0))
    _, whole, _, _ = run(dens, c, radii)
    for segment in (5, 11, 12, 2 ** 40):   # (12 blocks: inside them, the last, behind them, beyond 32 bits)
        got, info, _, _ = run(dens, c, radii, segment, 0)
        assert (got == want[:3]).all(), segment
        assert info[:2] == whole[:2], "the tile counts of the whole call"


@pytest.mark.parametrize("flaw", ["nan row", "inf row", "1e20 row"])
def test_flagged_data_is_answered_by_the_direct_kernel(dens, oracle, flaw):
    radii = std_radii(100)
    c = ref.stretched(300, 100).copy()
    if flaw == "nan row":
        c[131, 7] = np.nan
    elif flaw == "inf row":
        c[40, 99] = np.inf
    else:
        c[200, 0] = np.float32(1e20)
    for segment in (0, 2):   # (no segments: the whole sweep, whatever the segment argument holds)
        got, info, perm, _ = run(dens, c, radii, segment, 0, finite=False)
        assert info == (0, 0, 0)
        assert (got == oracle.populations(c, list(radii))).all()
    # as a segment: the row block dc_hip_populations_segment_dev answers for
    for seg, nseg in ((0, 3), (2, 3)):
        lo, hi = seg * (300 // nseg), (300 if seg == nseg - 1 else (seg + 1) * (300 // nseg))
        got, info, _, _ = run(dens, c, radii, seg, nseg, finite=False)
        assert info == (0, 0, 0)
        assert (got == oracle.populations(c, list(radii), lo, hi)).all(), (seg, nseg)
    # ... and the next call on clean data in the same workspace runs on the matrix cores again
    c, want = reference(300, 100, radii)
    check(dens, c, radii, want)


def test_a_small_call_behind_a_large_one_in_the_same_workspace(dens):
    c, want = reference(8320, 80, std_radii(80) + (1e-3, 0.0))
    check(dens, c, std_radii(80), want[:3])
    c, want = reference(300, 100, std_radii(100))
    check(dens, c, std_radii(100), want)
    c, want = reference(300, 256, std_radii(256))
    check(dens, c, std_radii(256), want)


@pytest.mark.parametrize("n_cols", [65, 256])
def test_at_most_one_percent_of_the_evaluated_pairs_go_to_the_exact_path(dens, n_cols):
    radii = std_radii(n_cols)
    c, want = reference(1500, n_cols, radii)
    (tiles, mfmas, exact), _, _ = check(dens, c, radii, want)
    print(f"D={n_cols}: {tiles} tile pairs, {exact} exact pairs = {100.0 * exact / (1024 * tiles):.4f} % of the evaluated pairs")
    assert exact <= 0.01 * 1024 * tiles


def test_the_order_of_another_shape_is_refused(dens):
    import ctypes as C
    import torch
    from clustering_amd import capi
    c, want = reference(300, 100, std_radii(100))
    check(dens, c, std_radii(100), want)
    ws = dens._wide_pruned_workspace(torch.device("cuda", torch.cuda.current_device())).buf
    perm = torch.empty(300, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    assert capi.lib.dc_hip_wide_pruned_order_dev(p(ws), 300, 100, p(perm), None) == 0
    assert capi.lib.dc_hip_wide_pruned_order_dev(p(ws), 299, 100, p(perm), None) == -1
    assert capi.lib.dc_hip_wide_pruned_order_dev(p(ws), 300, 101, p(perm), None) == -1
    blank = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    assert capi.lib.dc_hip_wide_pruned_order_dev(p(blank), 300, 100, p(perm), None) == -1
