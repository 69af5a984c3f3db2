"""GPU: the pruned neighbour sweep at 257..1024 columns (density.nearest_neighbors_xwide_pruned) against the CPU oracle, bit
for bit on all four arrays: nn_idx, nn_d2 bits, hd_idx, hd_d2 bits.  Every finite case asserts the pruning check, a condition
on the counters: with boxes, gaps, bounds and free-energy ranges formed in float64 from the device's own order
(xwide_pruned_order), 16 |lower| <= tiles <= 16 |upper| and mfmas == tiles x ceil((2 + 3 D) / 16).  Cases and bounds:
tests/xwidepruneref.py (their premises are checked on the CPU by tests/test_xwide_pruned_cases.py)."""
import functools

import numpy as np
import pytest

import fe_families
import wideref
import widepruneref as pr
import widennpruneref as nnref
import xwidepruneref as ref
import xwideref

pytestmark = pytest.mark.gpu
F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
FAMILIES = ("pops", "ties_ulp", "constant", "gradient", "inf", "signed_zero", "nan")


@pytest.fixture(scope="module")
def dens():
    import torch
    assert torch.cuda.is_available()
    from clustering_amd import density
    return density


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def u64(t):
    return t.cpu().numpy().astype(np.uint32).astype(np.uint64)


def words(idx, d2):
    """(d2 bits << 32 | index) per row: partial results merge by its minimum"""
    return (bits(d2).astype(np.uint64) << np.uint64(32)) | np.asarray(idx, dtype=np.uint64)


def as_numpy(got):
    return u64(got[0]), got[1].cpu().numpy(), u64(got[2]), got[3].cpu().numpy()


def run(dens, c, fe, segment=0, n_segments=0, finite=True, want=None):
    """one call -> ((nn_idx, nn_d2, hd_idx, hd_d2) as numpy, (tiles, mfmas, exact), order, (lower, upper, ring-1 lower, upper)
    of the tile counter); want: the four arrays of the whole call, compared BEFORE the counters are"""
    import torch
    ct = torch.from_numpy(c).cuda()
    ft = torch.from_numpy(np.ascontiguousarray(fe, dtype=np.float32)).cuda()
    got = as_numpy(dens.nearest_neighbors_xwide_pruned(ct, ft, segment, n_segments))
    info = dens.xwide_pruned_info(ct.device)
    perm = dens.xwide_pruned_order(ct.device).cpu().numpy().astype(np.int64)
    assert sorted(perm.tolist()) == list(range(len(c))), "the order is a permutation of the rows"
    if want is not None:
        same(got, want, c.shape)
    if not finite:
        return got, info, perm, None
    bounds = tuple(16 * v for v in ref.nn_pair_bounds(c, fe, perm, segment, n_segments))
    lo, hi = bounds[:2]
    print(f"{c.shape} segment {segment}/{n_segments}: tiles {info[0]} in [{lo}, {hi}] (ring 1: [{bounds[2]}, {bounds[3]}]), "
          f"all {16 * pr.n_blocks(len(c)) ** 2}, exact pairs {info[2]}")
    if lo > 0:
        assert info[0] > 0 and info[1] > 0, "the matrix-core kernel did not answer"
    assert lo <= info[0] <= hi, "the pruning check"
    assert info[1] == info[0] * ref.mfmas_per_tile_pair(c.shape[1])
    return got, info, perm, bounds


def same(got, want, what=""):
    assert (got[0] == want[0]).all(), ("nn_idx", what)
    assert (bits(got[1]) == bits(want[1])).all(), ("nn_d2", what)
    assert (got[2] == want[2]).all(), ("hd_idx", what)
    assert (bits(got[3]) == bits(want[3])).all(), ("hd_d2", what)


def check(dens, c, fe, want):
    got, info, perm, bounds = run(dens, c, fe, want=want)
    return info, perm, bounds


@pytest.mark.parametrize("n_cols", ref.COLS)
def test_column_counts(dens, n_cols):
    import torch
    c, fe, want = ref.nn_case(300, n_cols)
    check(dens, c, fe, want)
    # ... and the unpruned call of these widths gives the same four arrays
    plain = dens.nearest_neighbors_xwide(torch.from_numpy(c).cuda(), torch.from_numpy(fe).cuda())
    same(as_numpy(plain), want, "nearest_neighbors_xwide")


@pytest.mark.parametrize("n_rows,n_cols", [(1, 300), (33, 300), (129, 300), (700, 300), (1500, 300), (2100, 300), (8320, 257)])
def test_row_counts_from_one_frame_to_a_second_launch_group(dens, n_rows, n_cols):
    c, fe, want = ref.nn_case(n_rows, n_cols)
    info, perm, (lo, hi, _, _) = check(dens, c, fe, want)
    if n_rows >= 700:
        assert hi < 16 * pr.n_blocks(n_rows) ** 2, "pruning happened"
    if n_rows == 1:
        assert int(want[0][0]) == 2 and want[1][0] == FLT_MAX and info[0] == 16
    if n_rows == 8320:
        assert pr.shares(pr.n_blocks(n_rows)) == 8 and info[0] > 0


@pytest.mark.parametrize("shape", sorted(ref.NN_TABLE))
def test_the_shapes_of_the_table_prune(dens, shape):
    c, fe, want = ref.nn_case(*shape)
    info, perm, (lo, hi, _, _) = check(dens, c, fe, want)
    assert hi < 16 * ref.NN_TABLE[shape][1]
    if shape[0] == 1500:
        print(f"D={shape[1]}: {info[2]} exact pairs = {100.0 * info[2] / (1024 * info[0]):.3f} % of the evaluated pairs")


@functools.lru_cache(maxsize=None)
def family_case(family):
    from oracle.oracle import Oracle
    o = Oracle()
    c = ref.stretched(2100, 300)
    pops = o.populations(c, [ref.base_radius(300)])[0]
    fe = fe_families.make(family, c, pops)
    return c, fe, o.nearest_neighbors(c, fe)


@pytest.mark.parametrize("family", FAMILIES)
def test_free_energies_of_every_family(dens, family):
    c, fe, want = family_case(family)
    if family == "nan":
        got, info, _, _ = run(dens, c, fe, finite=False)
        assert info == (0, 0, 0), "a NaN free energy flags the data: the direct kernel answers"
        same(got, want, family)
        return
    info, perm, (lo, hi, s1_lo, s1_hi) = check(dens, c, fe, want)
    if family == "constant":
        assert (want[2] == len(c) + 1).all() and (want[3] == FLT_MAX).all(), "no hd anywhere"
        assert (lo, hi) == (s1_lo, s1_hi), "ring 2 is empty: the counter is ring 1's"
    if family == "pops":
        top = int(np.argmin(fe))
        assert int(want[2][top]) == len(c) + 1 and want[3][top] == FLT_MAX, "the global minimum has no lower neighbour"
        qb = int(np.nonzero(perm == top)[0][0]) // ref.BLOCK
        assert ref.block_counts(c, fe, perm)[qb][0] == pr.n_blocks(len(c)), "... and its block sweeps everything"


def test_ties_go_to_the_lowest_row(dens, oracle):
    c, stars, dups = wideref.ties_case(300, 300)
    c = c.copy()
    c[:, :2] *= F32(ref.STRETCH)   # (the stretched layout; a power of two: the stars stay stars)
    c = np.ascontiguousarray(c)
    for name, fe in sorted(wideref.fe_families(len(c)).items()):
        want = oracle.nearest_neighbors(c, fe)
        check(dens, c, fe, want)
        for q, ring in stars:
            assert int(want[0][q]) == min(ring), name
        for copy, orig in dups:
            assert want[1][copy] == 0.0 and want[1][orig] == 0.0


@pytest.mark.parametrize("n_cols", [300, 1024])
def test_a_tie_across_blocks_is_decided_on_rows_not_on_positions(dens, oracle, n_cols):
    c, fe, (a, p, q) = nnref.cross_block_tie_case(n_cols)
    want = oracle.nearest_neighbors(c, fe)
    (got, info, perm, _) = run(dens, c, fe)
    pos = {int(r): k for k, r in enumerate(perm)}
    assert pos[p] // 128 == 0 and pos[a] // 128 == 1 and pos[q] // 128 == 2, "the premise, from the device's order"
    assert int(got[0][a]) == q and int(got[2][a]) == q, "the least (d2, ROW); a merge on positions answers p"
    assert got[1][a] == 9.0 and got[3][a] == 9.0
    same(got, want)


@pytest.mark.parametrize("n_cols", [300, 1024])
def test_the_margin_at_its_sharpest(dens, oracle, n_cols):
    tiles = {}
    for which in (-1, 0, 1):
        c, fe, (a, a2), gap2 = nnref.margin_case(which, n_cols)
        want = oracle.nearest_neighbors(c, fe)
        info, perm, (lo, hi, _, _) = check(dens, c, fe, want)
        for b, g in enumerate((0, 2, 4)):
            assert sorted(perm[128 * b:128 * (b + 1)].tolist()) == sorted(list(range(g, 384, 6)) + list(range(g + 1, 384, 6))), \
                "each group fills one block"
        assert (lo, hi) == (16 * 7, 16 * 8) and int(want[0][a]) == a2 and want[1][a] == 9.0
        tiles[which] = info[0]
    # seed pairs: 2 + 3 + 2; the far block joins ring 1 of block 0 only where its gap is BELOW far2_nn = fl(1.0001f x 9): the
    # pair one ulp inside is met, the pair on the bound is not counted
    assert tiles == {-1: 16 * 8, 0: 16 * 7, 1: 16 * 7}


@pytest.mark.parametrize("n_segments", [2, 3, 5, 40])
def test_segments_of_the_order(dens, n_segments):
    c, fe, want = ref.nn_case(1500, 300)
    none_idx = len(c) + 1
    merged = [np.full(len(c), np.iinfo(np.uint64).max, dtype=np.uint64) for _ in range(2)]
    tiles = mfmas = 0
    for seg in range(n_segments):
        got, info, perm, bounds = run(dens, c, fe, seg, n_segments)
        blocks = list(pr.segment_blocks(len(c), seg, n_segments))
        mine = np.zeros(len(c), dtype=bool)
        if blocks:
            mine[np.concatenate([perm[128 * b:128 * (b + 1)] for b in blocks])] = True
        else:
            assert info == (0, 0, 0) and bounds[:2] == (0, 0), "a segment without a block"
        assert (got[0][~mine] == none_idx).all() and (got[2][~mine] == none_idx).all(), "none outside the rows of its blocks"
        assert (got[1][~mine] == FLT_MAX).all() and (got[3][~mine] == FLT_MAX).all()
        for k in range(4):
            assert (bits(got[k][mine]) == bits(want[k][mine])).all() if k % 2 else (got[k][mine] == want[k][mine]).all(), \
                "the final results of its rows"
        merged[0] = np.minimum(merged[0], words(got[0], got[1]))
        merged[1] = np.minimum(merged[1], words(got[2], got[3]))
        tiles += info[0]
        mfmas += info[1]
    assert (merged[0] == words(want[0], want[1])).all() and (merged[1] == words(want[2], want[3])).all()
    whole = run(dens, c, fe)[1]
    assert (tiles, mfmas) == whole[:2], "the tile counts add up to those of the whole call"


def test_no_segments_is_the_whole_sweep_whatever_the_segment_argument_holds(dens):
    c, fe, want = ref.nn_case(700, 300)
    whole = run(dens, c, fe)[1]
    for segment in (3, 6, 2 ** 40):
        got, info, _, _ = run(dens, c, fe, segment, 0)
        same(got, want, segment)
        assert info[:2] == whole[:2]


@pytest.mark.parametrize("n_cols", [257, 1024])
def test_nothing_to_prune(dens, n_cols):
    import torch
    from oracle.oracle import Oracle
    o = Oracle()
    c, radii, _, _ = xwideref.band_case(n_cols)
    fe = o.free_energies(o.populations(c, [radii[0]])[0])
    want = o.nearest_neighbors(c, fe)
    info, perm, bounds = check(dens, c, fe, want)
    ct, ft = torch.from_numpy(c).cuda(), torch.from_numpy(fe).cuda()
    same(as_numpy(dens.nearest_neighbors_xwide(ct, ft)), want, "nearest_neighbors_xwide")
    plain_info = dens.xwide_sweep_info(ct.device)
    # The radius of this case prunes nothing in the population sweep (tests/test_gpu_xwide_pruned.py: the counters of the
    # unpruned sweep).  The neighbour rule starts from the nearest-neighbour distances, which are smaller: at 257 columns
    # the outer blobs lie further apart in the plane than that, and the float64 bounds -- which every finite case is held
    # to -- put 2 176 of the 2 304 tile pairs in BOTH lower and upper (measured: 2 176).  So the counters are the unpruned
    # sweep's wherever the bounds say that every block pair is met, and never above them.
    all_tiles = 16 * pr.n_blocks(len(c)) ** 2
    assert plain_info[0] == all_tiles and info[0] <= plain_info[0] and info[1] <= plain_info[1]
    if bounds[0] == all_tiles:
        assert info[:2] == plain_info[:2], "every block pair is met: the counters of the unpruned sweep"
    print(f"D={n_cols}: exact pairs {info[2]} = {100.0 * info[2] / (1024 * info[0]):.3f} % of the evaluated pairs "
          f"(unpruned {plain_info[2]})")
    assert info[2] <= 0.05 * 1024 * info[0]


@pytest.mark.parametrize("n_cols", [300, 500])   # (beyond 400 columns the column-chunked direct kernel answers)
@pytest.mark.parametrize("flaw", ["nan cell", "inf cell", "1e20 row"])
def test_flagged_coordinates_are_answered_by_the_direct_kernel(dens, oracle, flaw, n_cols):
    c, fe, _ = ref.nn_case(300, n_cols)
    c = c.copy()
    if flaw == "nan cell":
        c[131, 7] = np.nan
    elif flaw == "inf cell":
        c[40, n_cols - 1] = np.inf
    else:
        c[200, 0] = np.float32(1e20)
    got, info, _, _ = run(dens, c, fe, finite=False)
    assert info == (0, 0, 0)
    same(got, oracle.nearest_neighbors(c, fe), flaw)
    # as a segment: the row block dc_hip_nearest_neighbors_segment_dev answers for, "none" elsewhere
    for seg, nseg in ((0, 3), (2, 3)):
        lo, hi = seg * (300 // nseg), (300 if seg == nseg - 1 else (seg + 1) * (300 // nseg))
        got, info, _, _ = run(dens, c, fe, seg, nseg, finite=False)
        assert info == (0, 0, 0)
        same(got, oracle.nearest_neighbors(c, fe, lo, hi), (flaw, seg, nseg))
    # ... and the next call on clean data in the same workspace runs on the matrix cores again
    c, fe, want = ref.nn_case(300, n_cols)
    info, _, _ = check(dens, c, fe, want)
    assert info[0] > 0


def test_both_sweeps_in_one_workspace_in_either_order(dens):
    import torch
    c, fe, want = ref.nn_case(1500, 300)
    _, radii, pops = ref.pop_case(1500, 300, (1e-3, 0.0))
    ct = torch.from_numpy(c).cuda()
    check(dens, c, fe, want)
    assert (u64(dens.calculate_populations_xwide_pruned(ct, list(radii))) == pops).all()
    assert dens.xwide_pruned_info(ct.device)[0] > 0
    check(dens, c, fe, want)
    assert (u64(dens.calculate_populations_xwide_pruned(ct, list(radii))) == pops).all()


def test_a_small_call_behind_a_large_one_in_the_same_workspace(dens):
    c, fe, want = ref.nn_case(8320, 257)
    check(dens, c, fe, want)
    for n_cols in (300, 1024, 257):
        c, fe, want = ref.nn_case(300, n_cols)
        check(dens, c, fe, want)


CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from clustering_amd import capi, density as dens
from oracle.oracle import Oracle
import wideref, xwidepruneref as ref
ORDER = sys.argv[2]
assert capi.lib.dc_hip_canon_order().decode() == ORDER
o = Oracle(order=ORDER)
bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
u64 = lambda t: t.cpu().numpy().astype(np.uint32).astype(np.uint64)
for n in (300, 700):
    ties = wideref.ties_case(n, 300)[0].copy()
    ties[:, :2] *= np.float32(ref.STRETCH)
    for c in (ref.stretched(n, 300), np.ascontiguousarray(ties)):
        fe = o.free_energies(o.populations(c, [ref.base_radius(300)])[0])
        exp = o.nearest_neighbors(c, fe)
        ct = torch.from_numpy(c).cuda()
        g = dens.nearest_neighbors_xwide_pruned(ct, torch.from_numpy(fe).cuda())
        assert dens.xwide_pruned_info(ct.device)[0] > 0
        assert (u64(g[0]) == exp[0]).all() and (u64(g[2]) == exp[2]).all(), (n, "nn idx")
        assert (bits(g[1].cpu().numpy()) == bits(exp[1])).all() and (bits(g[3].cpu().numpy()) == bits(exp[3])).all(), (n, "nn d2")
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
