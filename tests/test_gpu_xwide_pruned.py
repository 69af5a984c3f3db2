"""GPU: the pruned population sweep at 257..1024 columns (density.calculate_populations_xwide_pruned) against the CPU
oracle, bit for bit.  Every finite case asserts the pruning check, a condition on the counters: with the block boxes formed
in float64 from the device's own order (xwide_pruned_order), every launch evaluates at least the block pairs with
gap^2 < r2max and at most those with gap^2 < 1.001 r2max, 16 tile pairs each, and mfmas == tiles x ceil((2 + 3 D) / 16).
Cases: tests/xwidepruneref.py (their premises are checked on the CPU by tests/test_xwide_pruned_cases.py)."""
import numpy as np
import pytest

import widepruneref as pr
import xwidepruneref as ref
import xwideref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dens():
    import torch
    assert torch.cuda.is_available()
    from clustering_amd import density
    return density


def u64(t):
    return t.cpu().numpy().astype(np.uint32).astype(np.uint64)


def run(dens, c, radii, segment=0, n_segments=0, finite=True, want=None):
    """one call -> (populations as uint64, (tiles, mfmas, exact), order, (lower, upper) of the tile counter); want: the
    populations of the whole call, compared BEFORE the counters are (a wrong value is reported as one)"""
    import torch
    ct = torch.from_numpy(c).cuda()
    got = dens.calculate_populations_xwide_pruned(ct, list(radii), segment, n_segments)
    info = dens.xwide_pruned_info(ct.device)
    perm = dens.xwide_pruned_order(ct.device).cpu().numpy().astype(np.int64)
    assert sorted(perm.tolist()) == list(range(len(c))), "the order is a permutation of the rows"
    if want is not None:
        assert (u64(got) == want).all(), ("populations", c.shape, radii)
    if not finite:
        return u64(got), info, perm, None
    lo, hi = pr.tile_bounds(c, perm, list(radii), segment, n_segments)
    print(f"{c.shape} radii={len(radii)} segment {segment}/{n_segments}: tiles {info[0]} in [{lo}, {hi}], "
          f"all {16 * pr.n_blocks(len(c)) ** 2 * len(pr.launch_r2max(list(radii)))}, exact pairs {info[2]}")
    if lo > 0:
        assert info[0] > 0 and info[1] > 0, "the matrix-core kernel did not answer"
    assert lo <= info[0] <= hi, "the pruning check"
    assert info[1] == info[0] * ref.mfmas_per_tile_pair(c.shape[1])
    return u64(got), info, perm, (lo, hi)


def check(dens, c, radii, want):
    got, info, perm, bounds = run(dens, c, radii, want=want)
    return info, perm, bounds


@pytest.mark.parametrize("n_cols", ref.COLS)
def test_column_counts(dens, n_cols):
    c, radii, want = ref.pop_case(300, n_cols)
    check(dens, c, radii, want)


@pytest.mark.parametrize("n_rows,n_cols", [(1, 300), (33, 300), (129, 300), (700, 300), (1500, 300), (2100, 300), (8320, 257)])
def test_row_counts_from_one_frame_to_a_second_launch_group(dens, n_rows, n_cols):
    c, radii, want = ref.pop_case(n_rows, n_cols, (1e-3, 0.0))
    info, perm, (lo, hi) = check(dens, c, radii[:3], want[:3])
    if n_rows in ref.POP_TABLE or n_rows == 8320:
        assert hi < 16 * pr.n_blocks(n_rows) ** 2, "pruning happened"
    if n_rows == 1:
        assert int(want[0][0]) == 1 and info[0] == 16


def test_shares_without_a_survivor(dens):
    # 8 320 rows: 65 blocks in 8 shares; at these radii a query block meets the blocks whose boxes touch its own, so
    # (query block, share) units are left without a survivor -- they run no chain and still add the frames' own 1 (share 0)
    c, _, want = ref.pop_case(8320, 257, (1e-3, 0.0))
    radii = [1e-3, 0.0]
    info, perm, (lo, hi) = check(dens, c, radii, want[3:])
    nb = pr.n_blocks(len(c))
    assert nb == 65 and pr.shares(nb) == 8 and info[0] >= 16 * nb
    empty, units = pr.empty_units(c, perm, pr.launch_r2max(radii)[0])
    print(f"{empty} of {units} (query block, share) units without a survivor")
    assert units == 8 * nb and empty > 0, "the premise, from the device's order: there are such units"
    assert (want[3:] >= 1).all() and (want[4] == 1).all()


@pytest.mark.parametrize("n_cols", [300, 1024])
def test_the_margin_at_its_sharpest(dens, oracle, n_cols):
    c, r, (a, b, cc, d) = pr.margin_case(n_cols)
    want = oracle.populations(c, [r])
    info, perm, bounds = check(dens, c, [r], want)
    assert sorted(perm[:128].tolist()) == list(range(0, 256, 2)) and sorted(perm[128:].tolist()) == list(range(1, 256, 2)), \
        "each group fills one block"
    assert bounds == (64, 64) and info[0] == 64, "the block pair whose box gap is one ulp inside the radius is met"
    assert info[2] > 0, "pairs exactly on a radius can only be decided by the exact path"
    x = c.astype(np.float64)
    d2 = ((x[a][None, :] - x) ** 2).sum(axis=1)
    assert d2[d] < 9.0 and d2[b] == 9.0 and d2[cc] > 9.0
    assert int(want[0][a]) == int((d2 < 9.0).sum()), "a itself, d, and whatever else lies inside; not b, not c"
    # 8 and 11 radii with 0, 1e-3 and 1e30 among them: the second is two launches, and the counters add
    eight, eleven = pr.edge_radii(n_cols)
    want8 = oracle.populations(c, eight)
    info8, _, bounds8 = check(dens, c, eight, want8)
    info11, _, bounds11 = check(dens, c, eleven, oracle.populations(c, eleven))
    nm = ref.mfmas_per_tile_pair(n_cols)
    assert bounds8 == (64, 64) and bounds11 == (128, 128), "two launches: the counters add up to the sum of the two bounds"
    assert info8[:2] == (64, 64 * nm) and info11[:2] == (128, 128 * nm)
    assert (want8[eight.index(1e30)] == len(c)).all() and (want8[eight.index(0.0)] == 1).all()


@pytest.mark.parametrize("n_cols", [257, 1024])
def test_nothing_to_prune(dens, n_cols):
    import torch
    c, radii, bound, pairs = xwideref.band_case(n_cols)
    from oracle.oracle import Oracle
    want = Oracle().populations(c, radii)
    info, perm, bounds = check(dens, c, radii, want)
    ct = torch.from_numpy(c).cuda()
    plain = dens.calculate_populations_xwide(ct, list(radii))
    plain_info = dens.xwide_sweep_info(ct.device)
    assert (u64(plain) == want).all()
    nb = pr.n_blocks(len(c))
    assert info[:2] == plain_info[:2] == (16 * nb * nb, 16 * nb * nb * ref.mfmas_per_tile_pair(n_cols))
    print(f"D={n_cols}: exact pairs {info[2]} (unpruned {plain_info[2]}), bound {bound} of {pairs} pairs")
    assert info[2] <= bound


@pytest.mark.parametrize("n_cols", ref.TABLE_COLS)
def test_the_exact_path_of_the_stretched_case_stays_inside_its_bound(dens, n_cols):
    c, radii, want = ref.pop_case(1500, n_cols)
    (tiles, mfmas, exact), _, (lo, hi) = check(dens, c, radii, want)
    bound = ref.stretched_band_bound(n_cols)
    print(f"D={n_cols}: {tiles} tile pairs, {exact} exact pairs = {100.0 * exact / (1024 * tiles):.4f} % of the evaluated pairs, bound {bound}")
    assert hi < 16 * 144 and exact <= bound


@pytest.mark.parametrize("n_segments", [2, 3, 5, 40])
def test_segments_of_the_order(dens, n_segments):
    c, radii, want = ref.pop_case(1500, 300, (1e-3, 0.0))
    radii, want = radii[:3], want[:3]
    _, whole, _, _ = run(dens, c, radii)
    total = np.zeros_like(want)
    tiles = mfmas = 0
    for seg in range(n_segments):
        got, info, perm, bounds = run(dens, c, radii, seg, n_segments)
        blocks = list(pr.segment_blocks(len(c), seg, n_segments))
        rows = np.concatenate([perm[128 * b:128 * (b + 1)] for b in blocks]) if blocks else np.zeros(0, dtype=np.int64)
        mine = np.zeros(len(c), dtype=bool)
        mine[rows] = True
        assert (got[:, ~mine] == 0).all(), "zero outside the rows of its blocks"
        assert (got[:, mine] == want[:, mine]).all(), "the final counts of its rows"
        if not blocks:
            assert info == (0, 0, 0) and bounds == (0, 0), "a segment without a block"
        total += got
        tiles += info[0]
        mfmas += info[1]
    assert (total == want).all()
    assert (tiles, mfmas) == whole[:2], "the tile counts add up to those of the whole call"


def test_no_segments_is_the_whole_sweep_whatever_the_segment_argument_holds(dens):
    c, radii, want = ref.pop_case(1500, 300, (1e-3, 0.0))
    _, whole, _, _ = run(dens, c, radii[:3])
    for segment in (5, 11, 12, 2 ** 40):   # (12 blocks: inside them, the last, behind them, beyond 32 bits)
        got, info, _, _ = run(dens, c, radii[:3], segment, 0)
        assert (got == want[:3]).all(), segment
        assert info[:2] == whole[:2], "the tile counts of the whole call"


@pytest.mark.parametrize("n_cols", [300, 500])   # (beyond 400 columns the column-chunked direct kernel answers)
@pytest.mark.parametrize("flaw", ["nan cell", "inf cell", "1e20 row"])
def test_flagged_data_is_answered_by_the_direct_kernel(dens, oracle, flaw, n_cols):
    radii = ref.radii_for(n_cols)
    c = ref.stretched(300, n_cols).copy()
    if flaw == "nan cell":
        c[131, 7] = np.nan
    elif flaw == "inf cell":
        c[40, n_cols - 1] = np.inf
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
    c, radii, want = ref.pop_case(300, n_cols)
    info, _, _ = check(dens, c, radii, want)
    assert info[0] > 0


def test_a_small_call_behind_a_large_one_in_the_same_workspace(dens):
    c, radii, want = ref.pop_case(8320, 257, (1e-3, 0.0))
    check(dens, c, radii[:3], want[:3])
    for n_cols in (300, 1024, 257):
        c, radii, want = ref.pop_case(300, n_cols)
        check(dens, c, radii, want)


def test_the_order_of_another_shape_is_refused(dens):
    import ctypes as C
    import torch
    from clustering_amd import capi
    c, radii, want = ref.pop_case(300, 300)
    check(dens, c, radii, want)
    ws = dens._cached("xwide_pruned", torch.device("cuda", torch.cuda.current_device())).buf
    perm = torch.empty(300, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    order = capi.lib.dc_hip_xwide_pruned_order_dev
    assert order(p(ws), 300, 300, p(perm), None) == 0
    assert order(p(ws), 299, 300, p(perm), None) == -1
    assert order(p(ws), 300, 301, p(perm), None) == -1
    blank = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    assert order(p(blank), 300, 300, p(perm), None) == -1
    with pytest.raises(capi.DensityLibraryError):
        dens.calculate_populations_xwide_pruned(torch.zeros((10, 256), device="cuda"), [1.0])
    with pytest.raises(capi.DensityLibraryError):
        dens.calculate_populations_wide_pruned(torch.zeros((10, 257), device="cuda"), [1.0])


CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from clustering_amd import capi, density as dens
from oracle.oracle import Oracle
import widepruneref as pr, xwidepruneref as ref
ORDER = sys.argv[2]
assert capi.lib.dc_hip_canon_order().decode() == ORDER
o = Oracle(order=ORDER)
u64 = lambda t: t.cpu().numpy().astype(np.uint32).astype(np.uint64)
for n in (300, 700):
    c = ref.stretched(n, 300)
    radii = ref.radii_for(300)
    ct = torch.from_numpy(c).cuda()
    g = dens.calculate_populations_xwide_pruned(ct, radii)
    assert dens.xwide_pruned_info(ct.device)[0] > 0
    assert (u64(g) == o.populations(c, radii)).all(), n
c, r, _ = pr.margin_case(300)
g = dens.calculate_populations_xwide_pruned(torch.from_numpy(c).cuda(), [r])
assert (u64(g) == o.populations(c, [r])).all(), "margin"
print("ok")
"""


@pytest.mark.parametrize("order", ["avx", "fma"])
def test_the_libraries_of_the_other_summation_orders(order):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(root, "clustering_amd", "lib_" + order, "libdcdensity.so")):
        pytest.fail(f"clustering_amd/lib_{order}/libdcdensity.so is missing: __graft_entry__.build() makes it")
    env = dict(os.environ, DC_CANON_ORDER=order)
    env.pop("DC_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-c", CHILD, root, order], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
