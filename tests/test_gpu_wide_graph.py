"""GPU: the radius graph on the wide matrix-core sweep (density.radius_pairs_wide / radius_min_edge_wide /
radius_forest_wide, 65..256 columns) against brute force over the probe's canonical d2 matrix (tests/graphref.py), the
oracle's populations and the existing calls (dc_hip_radius_pairs_dev, dc_hip_radius_min_edge_segment_dev,
dc_hip_radius_forest), which run the direct kernels at these widths.  Every finite case first asserts that the
matrix-core kernel answered (wide_sweep_info: tiles > 0) -- a silent fall-back to the direct kernels would otherwise
pass.  Cases: tests/widegraphref.py (their premises are checked on the CPU by tests/test_wide_graph_cases.py)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import graphref
import wideref
import widegraphref as wg
from graphref import ALL_ONES, brute_pairs, check_forest, components, degrees, keys, min_edge_brute

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dens():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from clustering_amd import density
    return density


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw_pairs_wide(dens, ct, r2, capacity, rows=None):
    """graphref.raw_pairs for dc_hip_radius_pairs_wide_dev: a buffer of `rows` pairs (default: capacity) prefilled with
    -1, of which the library is told `capacity` -> (count, pairs int32 numpy [rows, 2] or None, pops, counters)"""
    import torch
    from clustering_amd import capi
    n, d = ct.shape
    rows = capacity if rows is None else rows
    assert rows >= capacity
    pops = torch.full((n,), -7, dtype=torch.int32, device=ct.device)
    count = torch.full((1,), -7, dtype=torch.int64, device=ct.device)
    pairs = torch.full((rows, 2), -1, dtype=torch.int32, device=ct.device) if rows else None
    ws, ws_bytes = dens._wide_workspace(ct.device).get(n, d, 1)
    with torch.cuda.device(ct.device):
        rc = capi.lib.dc_hip_radius_pairs_wide_dev(dens._dev(ct), n, d, float(r2), dens._dev(pops),
                                                   dens._dev(pairs) if pairs is not None else None, capacity,
                                                   dens._dev(count), ws, ws_bytes, dens._stream_ptr())
    capi.check(rc, "dc_hip_radius_pairs_wide_dev")
    torch.cuda.synchronize()
    info = dens.wide_sweep_info(ct.device) if n else (0, 0, 0)
    return int(count.item()), (pairs.cpu().numpy() if pairs is not None else None), pops.cpu().numpy(), info


@functools.lru_cache(maxsize=None)
def reference(case, *shape):
    """(coords, r, r2, brute-force pairs): computed once per case and shared by the tests that need it"""
    from oracle.oracle import Probe, build
    build()
    if case == "blobs":
        c, r, r2 = wg.blob_case(*shape)
    elif case == "sparse":
        c, r, r2 = wg.sparse_case()
    elif case == "boundary":
        c, r, _ = wideref.boundary_case(*shape)
        r2 = wg.square(r)
    else:
        c = wideref.ties_case(*shape)[0]
        r = wg.blob_radius(shape[1])
        r2 = wg.square(r)
    return c, r, r2, brute_pairs(Probe(), c, r2)


def check_pair_list(dens, oracle, c, r, r2, want):
    """the list, the populations and the count of one call -> the counters"""
    n = len(c)
    ct = cuda(c)
    pairs, pops = dens.radius_pairs_wide(ct, r2)
    info = dens.wide_sweep_info(ct.device)
    assert info[0] > 0 and info[1] > 0, "the matrix-core kernel did not answer"
    pairs = pairs.cpu().numpy()
    got = keys(pairs, n)
    assert len(np.unique(got)) == len(got), "a pair was listed twice"
    assert np.array_equal(np.sort(got), keys(want, n))
    assert (pairs[:, 0] != pairs[:, 1]).all() and ((pairs >= 0) & (pairs < n)).all()
    pops = pops.cpu().numpy().astype(np.int64)
    assert (pops == degrees(want, n)).all()
    if r is not None:
        assert (pops.astype(np.uint64) == oracle.populations(c, [r])[0]).all()
    count, _, pops_c, _ = raw_pairs_wide(dens, ct, r2, 0)
    assert count == len(want), "d_count is exact"
    assert (pops_c.astype(np.int64) == pops).all()
    return info


# ---- the pair list ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols", wg.COLS)
def test_pairs_at_column_counts_on_both_sides_of_the_chunk_seam(dens, oracle, n_cols):
    c, r, r2, want = reference("blobs", 200, n_cols)
    assert len(want) > 0
    check_pair_list(dens, oracle, c, r, r2, want)


@pytest.mark.parametrize("n_rows", wg.ROWS)
def test_pairs_from_one_frame_to_several_workgroups_and_shares(dens, oracle, n_rows):
    c, r, r2, want = reference("blobs", n_rows, 100)
    assert len(want) > 0 or n_rows <= 2
    info = check_pair_list(dens, oracle, c, r, r2, want)
    assert info[1] == 19 * info[0], "19 MFMAs per tile pair at 100 columns"


def test_pairs_of_the_sparse_case_across_shares_and_query_blocks(dens, oracle):
    c, r, r2, want = reference("sparse")
    assert len(wg.split_pairs(want, len(c))) > 100
    check_pair_list(dens, oracle, c, r, r2, want)


def test_pairs_on_and_one_ulp_to_either_side_of_the_radius(dens, oracle):
    c, r, r2, want = reference("boundary", 300, 80)
    assert r2 == np.float32(9.0)
    info = check_pair_list(dens, oracle, c, r, r2, want)
    assert info[2] > 0, "pairs exactly on a radius can only be decided by the exact path"
    pairs, _ = dens.radius_pairs_wide(cuda(c), r2)
    got = set(keys(pairs.cpu().numpy(), len(c)).tolist())
    for a, b, cc, d in wideref.boundary_case(300, 80)[2]:
        assert int(keys([[a, b]], len(c))[0]) not in got, "the pair on the radius"
        assert int(keys([[a, cc]], len(c))[0]) not in got, "the pair one ulp outside"
        assert int(keys([[a, d]], len(c))[0]) in got, "the pair one ulp inside"


def test_the_complete_graph_and_radii_that_hold_no_pair(dens, oracle):
    """r2 beyond every d2: n (n - 1) / 2 pairs -- the i < j rule inside diagonal tiles and the tile-level skip; r2 of
    NaN, 0 and -1: no pair, every population 1"""
    c = wideref.blobs(200, 100)
    n = len(c)
    ii, jj = np.triu_indices(n, 1)
    everything = np.stack([ii, jj], axis=1).astype(np.int64)
    for r2 in (1.0e6, 3.0e38, float("inf")):
        check_pair_list(dens, oracle, c, None, r2, everything)
    ct = cuda(c)
    for r2 in (float("nan"), 0.0, -0.0, -1.0, -float("inf")):
        count, part, pops, info = raw_pairs_wide(dens, ct, r2, 16)
        assert count == 0 and (part == -1).all() and (pops == 1).all(), r2
        assert info[0] > 0, "the matrix-core kernel answers these too"
        pairs, pops = dens.radius_pairs_wide(ct, r2)
        assert pairs.shape == (0, 2) and bool((pops == 1).all())


@pytest.mark.parametrize("case", [("blobs", 2100, 100), ("sparse",), ("boundary", 300, 80)])
def test_capacity(dens, case):
    """counting only; a third of the count: the full count, exactly `capacity` distinct valid pairs, the rows beyond
    untouched; exactly the count"""
    c, r, r2, want = reference(*case)
    n, total = len(c), len(want)
    assert total >= 3
    ct = cuda(c)
    want_keys = keys(want, n)
    count, part, pops, info = raw_pairs_wide(dens, ct, r2, 0)
    assert count == total and part is None and info[0] > 0
    assert (pops.astype(np.int64) == degrees(want, n)).all()
    short = total // 3
    count, part, pops, _ = raw_pairs_wide(dens, ct, r2, short, rows=short + 64)
    assert count == total, "the full count, whatever the capacity"
    assert (part[short:] == -1).all(), "nothing is written beyond the capacity"
    assert (part[:short] >= 0).all() and (part[:short, 0] != part[:short, 1]).all()
    assert np.isin(keys(part[:short], n), want_keys).all() and len(np.unique(keys(part[:short], n))) == short
    assert (pops.astype(np.int64) == degrees(want, n)).all()
    count, part, _, _ = raw_pairs_wide(dens, ct, r2, total, rows=total + 64)
    assert count == total and (part[total:] == -1).all()
    assert np.array_equal(np.sort(keys(part[:total], n)), want_keys)


def test_pairs_of_no_rows(dens):
    import torch
    count, part, pops, info = raw_pairs_wide(dens, torch.zeros((0, 100), device="cuda"), 1.0, 0)
    assert count == 0 and len(pops) == 0
    pairs, pops = dens.radius_pairs_wide(torch.zeros((0, 65), device="cuda"), 1.0)
    assert pairs.shape == (0, 2) and pops.shape == (0,)


# ---- one Boruvka round --------------------------------------------------------------------------------------------------
def u64(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("n_rows,n_cols", [(300, 100), (200, 256)])
def test_min_edge_round_for_every_labelling_and_rank(dens, n_rows, n_cols):
    """against the definition (min_edge_brute) on data with duplicated rows and rings of tied partners; whole rounds and,
    at 300 rows, 3 and 7 segments (row blocks that are no multiples of 128): every segment array-equal to
    dc_hip_radius_min_edge_segment_dev, and the merged partials equal to the whole round"""
    import torch
    c, r, r2, pairs = reference("ties", n_rows, n_cols)
    ct = cuda(c)
    deg = degrees(pairs, n_rows)
    for lab in ("own", "one", "any"):
        comp = graphref.labels(lab, n_rows)
        compt = cuda(comp.astype(np.int32))
        for kind in graphref.RANKS:
            rank = graphref.rank_of(kind, n_rows)
            rankt = cuda(rank.astype(np.int32))
            want = min_edge_brute(pairs, comp, rank, n_rows)
            best, pops = dens.radius_min_edge_wide(ct, r2, compt, rankt)
            assert dens.wide_sweep_info(ct.device)[0] > 0, "the matrix-core kernel did not answer"
            assert (u64(best) == want).all(), (lab, kind)
            assert (pops.cpu().numpy().astype(np.int64) == deg).all(), (lab, kind)
            assert ((want != ALL_ONES).any()) == (lab != "one")
            old_b, old_p = dens.radius_min_edge(ct, r2, compt, rankt)
            assert torch.equal(best, old_b) and torch.equal(pops, old_p), (lab, kind)
            if n_rows != 300:
                continue
            for n_seg in (3, 7):
                acc_b = np.full(n_rows, ALL_ONES, dtype=np.uint64)
                acc_p = np.zeros(n_rows, dtype=np.int64)
                for g in range(n_seg):
                    b, p = dens.radius_min_edge_wide(ct, r2, compt, rankt, g, n_seg)
                    assert dens.wide_sweep_info(ct.device)[0] > 0
                    ob, op = dens.radius_min_edge(ct, r2, compt, rankt, g, n_seg)
                    assert torch.equal(b, ob) and torch.equal(p, op), (lab, kind, g, n_seg)
                    acc_b = np.minimum(acc_b, u64(b))
                    acc_p += p.cpu().numpy().astype(np.int64)
                assert (acc_b == want).all() and (acc_p == deg).all(), (lab, kind, n_seg)


def test_min_edge_smallest_rank_rule_on_both_sides_of_the_query(dens):
    """a query whose lightest partner ranks ABOVE it and one whose lightest partner ranks BELOW it (counted by the
    referee), every frame its own component, across two shares"""
    c, r, r2, pairs = reference("blobs", 2100, 100)
    n = len(c)
    ct = cuda(c)
    comp = graphref.labels("own", n)
    for kind in ("identity", "random"):
        rank = graphref.rank_of(kind, n)
        higher, lower = wg.rank_rule_witnesses(pairs, comp, rank)
        assert higher > 0 and lower > 0
        best, pops = dens.radius_min_edge_wide(ct, r2, cuda(comp.astype(np.int32)), cuda(rank.astype(np.int32)))
        assert dens.wide_sweep_info(ct.device)[0] > 0
        assert (u64(best) == min_edge_brute(pairs, comp, rank, n)).all(), kind
        assert (pops.cpu().numpy().astype(np.int64) == degrees(pairs, n)).all()


def test_min_edge_radii_that_hold_no_pair(dens):
    c, r, r2, pairs = reference("ties", 300, 100)
    ct = cuda(c)
    comp, rank = cuda(graphref.labels("own", 300).astype(np.int32)), cuda(graphref.rank_of("random", 300).astype(np.int32))
    for none in (float("nan"), 0.0, -1.0):
        best, pops = dens.radius_min_edge_wide(ct, none, comp, rank)
        assert (u64(best) == ALL_ONES).all() and bool((pops == 1).all()), none


# ---- the forest ---------------------------------------------------------------------------------------------------------
def forest_cases():
    c, r2 = wg.chain_case(150, 65)
    yield "chain", c, r2
    c, r2, _, _, _ = graphref.bridge(100)
    yield "two cliques and a bridge", c, r2
    c = wideref.blobs(200, 100)
    yield "complete", c, 1.0e6
    yield "empty", c, 1.0e-6
    yield "blobs in two shares", reference("blobs", 2100, 100)[0], reference("blobs", 2100, 100)[2]


def test_forest_against_the_contract(dens, probe):
    for name, c, r2 in forest_cases():
        n = len(c)
        pairs = brute_pairs(probe, c, r2)
        for kind in ("random", "reversed"):
            rank = graphref.rank_of(kind, n)
            edges, rounds = dens.radius_forest_wide(c, r2, rank)
            n_comp = check_forest(n, pairs, rank, edges, rounds)
            assert n_comp == len(np.unique(components(n, pairs))), name
        if name == "empty":
            assert len(edges) == 0 and rounds == 1
        if name in ("chain", "complete", "two cliques and a bridge"):
            assert len(edges) == n - 1


def test_forest_of_no_one_and_two_rows(dens):
    for n in (0, 1, 2):
        c = np.zeros((n, 100), dtype=np.float32)
        if n == 2:
            c[1, 3] = 1.0
        edges, rounds = dens.radius_forest_wide(c, 2.0, np.arange(n, dtype=np.uint32))
        assert edges.shape == (max(n - 1, 0), 2) and rounds == (2 if n == 2 else 0)
        if n == 2:
            assert sorted(edges[0].tolist()) == [0, 1]
            edges, rounds = dens.radius_forest_wide(c, 1.0, np.arange(n, dtype=np.uint32))   # (d2 = 1 is not < 1)
            assert len(edges) == 0 and rounds == 1
    with pytest.raises(Exception, match="permutation"):
        dens.radius_forest_wide(np.zeros((3, 100), dtype=np.float32), 1.0, np.array([0, 1, 1], dtype=np.uint32))


def test_forest_has_the_connectivity_of_the_existing_call(dens):
    c, r, r2, pairs = reference("blobs", 1500, 100)
    n = len(c)
    rank = graphref.rank_of("random", n)
    edges, rounds = dens.radius_forest_wide(c, r2, rank)
    old, old_rounds = dens.radius_forest(c, r2, rank)
    assert len(edges) > 0 and len(edges) == len(old)
    assert (components(n, edges) == components(n, old)).all()
    check_forest(n, pairs, rank, edges, rounds)
    # (the lightest pair of a component is unique -- the ranks are a permutation -- so the two forests are one)
    assert np.array_equal(np.sort(keys(edges, n)), np.sort(keys(old, n))) and rounds == old_rounds


# ---- flagged data -------------------------------------------------------------------------------------------------------
def test_flagged_data_is_answered_by_the_direct_kernels(dens):
    import torch
    c, r, r2, _ = reference("blobs", 500, 100)
    c = wg.with_non_finite(c)
    n = len(c)
    ct = cuda(c)
    pairs, pops = dens.radius_pairs_wide(ct, r2)
    assert dens.wide_sweep_info(ct.device) == (0, 0, 0)
    old_pairs, old_pops = dens.radius_pairs(ct, r2)
    assert len(pairs) > 0 and torch.equal(pops, old_pops)
    assert np.array_equal(np.sort(keys(pairs.cpu().numpy(), n)), np.sort(keys(old_pairs.cpu().numpy(), n)))
    assert bool((pops[list(wg.FLAGGED_ROWS)] == 1).all())
    count, part, _, info = raw_pairs_wide(dens, ct, r2, len(pairs) // 3, rows=len(pairs))
    assert count == len(pairs) and info == (0, 0, 0) and (part[len(pairs) // 3:] == -1).all()
    comp, rank = cuda(graphref.labels("any", n).astype(np.int32)), cuda(graphref.rank_of("random", n).astype(np.int32))
    for seg, n_seg in ((0, 0), (1, 3)):
        best, p = dens.radius_min_edge_wide(ct, r2, comp, rank, seg, n_seg)
        assert dens.wide_sweep_info(ct.device) == (0, 0, 0)
        old_best, old_p = dens.radius_min_edge(ct, r2, comp, rank, seg, n_seg)
        assert torch.equal(best, old_best) and torch.equal(p, old_p)
    assert (u64(best) != ALL_ONES).any()
    edges, rounds = dens.radius_forest_wide(c, r2, graphref.rank_of("random", n))
    old, _ = dens.radius_forest(c, r2, graphref.rank_of("random", n))
    assert np.array_equal(np.sort(keys(edges, n)), np.sort(keys(old, n)))
    # ... and the next call on clean data in the same workspace runs on the matrix cores again
    c, r, r2, want = reference("blobs", 200, 100)
    count, _, _, info = raw_pairs_wide(dens, cuda(c), r2, 0)
    assert count == len(want) and info[0] > 0


# ---- the cap on the exact path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols", [65, 256])
def test_at_most_one_percent_of_the_pairs_reach_the_exact_path(dens, n_cols):
    c, r, r2 = wg.blob_case(1500, n_cols)
    ct = cuda(c)
    count, _, _, (tiles, mfmas, exact) = raw_pairs_wide(dens, ct, r2, 0)
    print(f"D={n_cols} pairs: {count} pairs, {tiles} tile pairs, {mfmas} MFMAs, {exact} exact pairs = "
          f"{100.0 * exact / (1024 * tiles):.4f} % of the evaluated pairs")
    assert tiles > 0 and exact <= 0.01 * 1024 * tiles
    comp, rank = cuda(graphref.labels("any", 1500).astype(np.int32)), cuda(graphref.rank_of("random", 1500).astype(np.int32))
    dens.radius_min_edge_wide(ct, r2, comp, rank)
    tiles, mfmas, exact = dens.wide_sweep_info(ct.device)
    print(f"D={n_cols} min edge: {exact} exact pairs = {100.0 * exact / (1024 * tiles):.4f} % of the evaluated pairs")
    assert tiles > 0 and exact <= 0.01 * 1024 * tiles


# ---- the libraries of the other summation orders ------------------------------------------------------------------------
CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from clustering_amd import capi, density as dens
from oracle.oracle import Probe
import graphref, wideref, widegraphref as wg
ORDER = sys.argv[2]
assert capi.lib.dc_hip_canon_order().decode() == ORDER
probe = Probe(order=ORDER)
u64 = lambda t: t.cpu().numpy().view(np.uint64)
for n, d in ((200, 65), (300, 100), (200, 256)):
    for c, r2 in ((wideref.ties_case(n, d)[0], wg.square(wg.blob_radius(d))), (wideref.boundary_case(n, d)[0], np.float32(9.0))):
        ct = torch.from_numpy(c).cuda()
        want = graphref.brute_pairs(probe, c, r2)
        assert len(want) > 0
        pairs, pops = dens.radius_pairs_wide(ct, r2)
        assert dens.wide_sweep_info(ct.device)[0] > 0
        got = graphref.keys(pairs.cpu().numpy(), n)
        assert len(np.unique(got)) == len(got) and np.array_equal(np.sort(got), graphref.keys(want, n)), (n, d, "pairs")
        assert (pops.cpu().numpy().astype(np.int64) == graphref.degrees(want, n)).all(), (n, d, "pops")
        for lab in ("own", "any"):
            comp, rank = graphref.labels(lab, n), graphref.rank_of("random", n)
            best, pops = dens.radius_min_edge_wide(ct, r2, torch.from_numpy(comp.astype(np.int32)).cuda(),
                                                   torch.from_numpy(rank.astype(np.int32)).cuda())
            assert dens.wide_sweep_info(ct.device)[0] > 0
            assert (u64(best) == graphref.min_edge_brute(want, comp, rank, n)).all(), (n, d, lab, "best")
            assert (pops.cpu().numpy().astype(np.int64) == graphref.degrees(want, n)).all(), (n, d, lab, "pops")
        rank = graphref.rank_of("bit-reversed", n)
        edges, rounds = dens.radius_forest_wide(c, r2, rank)
        graphref.check_forest(n, want, rank, edges, rounds)
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
