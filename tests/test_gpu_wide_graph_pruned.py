"""GPU: the PRUNED radius graph on the wide matrix-core sweep (density.radius_pairs_wide_pruned /
radius_min_edge_wide_pruned / radius_forest_wide_pruned, 65..256 columns) against brute force over the
probe's canonical d2 matrix (tests/graphref.py), the oracle's populations and the unpruned calls (radius_*_wide).  Every
finite case with r2 > 0 first asserts that the matrix-core kernel answered (wide_pruned_info: tiles > 0), and every pair
call is held to the pruning check, a condition on the counter: with the block boxes formed in float64 from the device's
own order (wide_pruned_order), 16 #{gap^2 < r2} <= tiles <= 16 #{gap^2 < 1.001 r2}.  Cases: tests/widegraphpruneref.py
(their premises are checked on the CPU by tests/test_wide_graph_pruned_cases.py)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import graphref
import widegraphpruneref as wgp
import widegraphref as wg
import widepruneref as ref
import wideref
from graphref import ALL_ONES, brute_pairs, check_forest, components, degrees, keys, min_edge_brute

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_PAIR = (float("nan"), 0.0, -0.0, -1.0, -float("inf"))


@pytest.fixture(scope="module")
def dens():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from clustering_amd import density
    return density


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def order_of(dens, ct):
    perm = dens.wide_pruned_order(ct.device).cpu().numpy().astype(np.int64)
    assert sorted(perm.tolist()) == list(range(len(ct))), "the order is a permutation of the rows"
    return perm


def raw_pairs(dens, ct, r2, capacity, rows=None):
    """one dc_hip_radius_pairs_wide_pruned_dev call with a buffer of `rows` pairs (default: capacity) prefilled with -1, of
    which the library is told `capacity` -> (count, pairs int32 numpy [rows, 2] or None, pops, counters)"""
    import torch
    from clustering_amd import capi
    n, d = ct.shape
    rows = capacity if rows is None else rows
    assert rows >= capacity
    pops = torch.full((n,), -7, dtype=torch.int32, device=ct.device)
    count = torch.full((1,), -7, dtype=torch.int64, device=ct.device)
    pairs = torch.full((rows, 2), -1, dtype=torch.int32, device=ct.device) if rows else None
    ws, ws_bytes = dens._wide_pruned_workspace(ct.device).get(n, d, 1)
    with torch.cuda.device(ct.device):
        rc = capi.lib.dc_hip_radius_pairs_wide_pruned_dev(dens._dev(ct), n, d, float(r2), dens._dev(pops),
                                                          dens._dev(pairs) if pairs is not None else None, capacity,
                                                          dens._dev(count), ws, ws_bytes, dens._stream_ptr())
    capi.check(rc, "dc_hip_radius_pairs_wide_pruned_dev")
    torch.cuda.synchronize()
    info = dens.wide_pruned_info(ct.device) if n else (0, 0, 0)
    return int(count.item()), (pairs.cpu().numpy() if pairs is not None else None), pops.cpu().numpy(), info


@functools.lru_cache(maxsize=None)
def reference(case, *shape):
    """(coords, r, r2, brute-force pairs): computed once per case and shared by the tests that need it"""
    from oracle.oracle import Probe, build
    build()
    if case == "stretched":
        c, r, r2 = wgp.stretched_case(*shape)
    elif case == "blobs":
        c, r, r2 = wg.blob_case(*shape)
    elif case == "boundary":
        c, r, _ = wideref.boundary_case(*shape)
        r2 = wg.square(r)
    elif case == "margin":
        c, r, _ = ref.margin_case()
        r2 = wg.square(r)
    elif case == "small radius":
        c, r, r2, _ = wgp.small_radius_case()
    else:
        c, r, r2, _ = wgp.min_edge_case()
    return c, r, r2, brute_pairs(Probe(), c, r2)


def check_counter(c, perm, r, r2, info, segment=0, n_segments=0):
    """the pruning check of one call -> (lower, upper)"""
    lo, hi = wgp.tile_bounds_r2(c, perm, r2, segment, n_segments)
    if r is not None:
        assert (lo, hi) == ref.tile_bounds(c, perm, [r], segment, n_segments)
    print(f"{c.shape} r2={float(r2):.6g} segment {segment}/{n_segments}: tiles {info[0]} in [{lo}, {hi}], "
          f"all {16 * ref.n_blocks(len(c)) ** 2}, exact pairs {info[2]}")
    assert lo <= info[0] <= hi, "the pruning check"
    assert info[1] == info[0] * ((2 + 3 * c.shape[1] + 15) // 16)
    return lo, hi


def check_pair_list(dens, oracle, c, r, r2, want):
    """the list, the populations, the count and the counter of one call -> (counters, order, bounds)"""
    n = len(c)
    ct = cuda(c)
    pairs, pops = dens.radius_pairs_wide_pruned(ct, r2)
    info = dens.wide_pruned_info(ct.device)
    assert info[0] > 0 and info[1] > 0, "the matrix-core kernel did not answer"
    perm = order_of(dens, ct)
    bounds = check_counter(c, perm, r, r2, info)
    pairs = pairs.cpu().numpy()
    got = keys(pairs, n)
    assert len(np.unique(got)) == len(got), "a pair was listed twice"
    assert np.array_equal(np.sort(got), keys(want, n))
    assert (pairs[:, 0] != pairs[:, 1]).all() and ((pairs >= 0) & (pairs < n)).all()
    pops = pops.cpu().numpy().astype(np.int64)
    assert (pops == degrees(want, n)).all()
    if r is not None:
        assert (pops.astype(np.uint64) == oracle.populations(c, [r])[0]).all()
    plain, plain_pops = dens.radius_pairs_wide(ct, r2)
    assert np.array_equal(np.sort(got), np.sort(keys(plain.cpu().numpy(), n))), "the set of radius_pairs_wide"
    assert (plain_pops.cpu().numpy().astype(np.int64) == pops).all()
    count, _, pops_c, info_c = raw_pairs(dens, ct, r2, 0)
    assert count == len(want), "d_count is exact"
    assert (pops_c.astype(np.int64) == pops).all() and info_c[:2] == info[:2]
    return info, perm, bounds


# ---- the pair list ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", wgp.STRETCHED)
def test_pairs_of_the_stretched_blobs_with_block_pairs_dropped(dens, oracle, shape):
    c, r, r2, want = reference("stretched", *shape)
    assert r == max(ref.radii_for(shape[1], 3)) and len(want) > 0
    info, perm, (lo, hi) = check_pair_list(dens, oracle, c, r, r2, want)
    nb = ref.n_blocks(len(c))
    assert 16 * ref.STRETCHED_TABLE[shape][0] < 16 * nb * nb and hi < 16 * nb * nb, "pruning happened"
    turned = wgp.pairs_against_the_order(want, perm)
    print(f"{shape}: {len(want)} pairs, {len(turned)} of them with their rows the other way round in the order")
    assert not np.array_equal(perm, np.arange(len(c))) and len(turned) > 0, "the premise, from the device's order"


def test_pairs_on_and_one_ulp_to_either_side_of_the_radius(dens, oracle):
    c, r, r2, want = reference("boundary", *wgp.BOUNDARY_SHAPE)
    assert r2 == np.float32(9.0)
    info, perm, _ = check_pair_list(dens, oracle, c, r, r2, want)
    assert info[2] > 0, "pairs exactly on a radius can only be decided by the exact path"
    pairs, _ = dens.radius_pairs_wide_pruned(cuda(c), r2)
    got = set(keys(pairs.cpu().numpy(), len(c)).tolist())
    for g, (a, b, cc, d) in enumerate(wideref.boundary_case(*wgp.BOUNDARY_SHAPE)[2]):
        blocks = wgp.blocks_of((a, b, cc, d), perm)
        assert (blocks[0] not in blocks[1:]) == (g in wgp.BOUNDARY_SPLIT_GROUPS), "the premise, from the device's order"
        assert int(keys([[a, b]], len(c))[0]) not in got, "the pair on the radius"
        assert int(keys([[a, cc]], len(c))[0]) not in got, "the pair one ulp outside"
        assert int(keys([[a, d]], len(c))[0]) in got, "the pair one ulp inside"


def test_the_margin_at_its_sharpest(dens, oracle):
    c, r, r2, want = reference("margin")
    a, b, cc, d = ref.margin_case()[2]
    info, perm, bounds = check_pair_list(dens, oracle, c, r, r2, want)
    assert wgp.blocks_of((a, b, cc, d), perm) == [0, 1, 1, 1]
    assert bounds == (64, 64) and info[0] == 64, "the block pair whose box gap is one ulp inside the radius is met"
    got = set(keys(want, len(c)).tolist())
    assert int(keys([[a, d]], len(c))[0]) in got and int(keys([[a, b]], len(c))[0]) not in got


@pytest.mark.parametrize("n_cols", wg.COLS)
def test_pairs_at_column_counts_on_both_sides_of_the_chunk_seam(dens, oracle, n_cols):
    c, r, r2, want = reference("blobs", 200, n_cols)
    assert len(want) > 0
    check_pair_list(dens, oracle, c, r, r2, want)


@pytest.mark.parametrize("n_rows", [1, 2, 33, 129])
def test_pairs_of_a_few_rows(dens, oracle, n_rows):
    c, r, r2, want = reference("blobs", n_rows, 100)
    assert len(want) > 0 or n_rows <= 2
    info, _, _ = check_pair_list(dens, oracle, c, r, r2, want)
    assert info[1] == 19 * info[0], "19 MFMAs per tile pair at 100 columns"


def test_units_without_a_survivor_still_add_the_frames_own_one(dens, oracle):
    c, r, r2, want = reference("small radius")
    dups = wgp.small_radius_case()[3]
    assert np.array_equal(np.sort(keys(want, len(c))), np.sort(keys(dups, len(c)))), "the duplicates and nothing else"
    info, perm, (lo, hi) = check_pair_list(dens, oracle, c, r, r2, want)
    empty, units = ref.empty_units(c, perm, float(r2))
    print(f"{empty} of {units} (query block, share) units without a survivor")
    assert units == 8 * 65 and empty > 0, "the premise, from the device's order"


def test_the_complete_graph_and_radii_that_hold_no_pair(dens, oracle):
    c = wideref.blobs(200, 100)
    n = len(c)
    ii, jj = np.triu_indices(n, 1)
    everything = np.stack([ii, jj], axis=1).astype(np.int64)
    for r2 in (1.0e6, 3.0e38, float("inf")):
        info, _, _ = check_pair_list(dens, oracle, c, None, r2, everything)
        assert info[0] == 16 * 4
    ct = cuda(c)
    for r2 in NO_PAIR:
        count, part, pops, info = raw_pairs(dens, ct, r2, 16)
        assert count == 0 and (part == -1).all() and (pops == 1).all(), r2
        assert info == (0, 0, 0), "no block pair can hold a pair: nothing is evaluated"
        pairs, pops = dens.radius_pairs_wide_pruned(ct, r2)
        assert pairs.shape == (0, 2) and bool((pops == 1).all())


@pytest.mark.parametrize("case", [("stretched", 2100, 100), ("boundary", 300, 80)])
def test_capacity(dens, case):
    """counting only; a third of the count: the full count, exactly `capacity` distinct valid pairs, the rows beyond
    untouched; exactly the count"""
    c, r, r2, want = reference(*case)
    n, total = len(c), len(want)
    assert total >= 3
    ct = cuda(c)
    want_keys = keys(want, n)
    count, part, pops, info = raw_pairs(dens, ct, r2, 0)
    assert count == total and part is None and info[0] > 0
    assert (pops.astype(np.int64) == degrees(want, n)).all()
    short = total // 3
    count, part, pops, _ = raw_pairs(dens, ct, r2, short, rows=short + 64)
    assert count == total, "the full count, whatever the capacity"
    assert (part[short:] == -1).all(), "nothing is written beyond the capacity"
    assert ((part[:short] >= 0) & (part[:short] < n)).all() and (part[:short, 0] != part[:short, 1]).all()
    assert np.isin(keys(part[:short], n), want_keys).all() and len(np.unique(keys(part[:short], n))) == short
    assert (pops.astype(np.int64) == degrees(want, n)).all()
    count, part, _, _ = raw_pairs(dens, ct, r2, total, rows=total + 64)
    assert count == total and (part[total:] == -1).all()
    assert np.array_equal(np.sort(keys(part[:total], n)), want_keys)


def test_pairs_of_no_rows(dens):
    import torch
    count, part, pops, info = raw_pairs(dens, torch.zeros((0, 100), device="cuda"), 1.0, 0)
    assert count == 0 and len(pops) == 0
    pairs, pops = dens.radius_pairs_wide_pruned(torch.zeros((0, 65), device="cuda"), 1.0)
    assert pairs.shape == (0, 2) and pops.shape == (0,)


# ---- one Boruvka round --------------------------------------------------------------------------------------------------
def test_min_edge_round_for_every_labelling_and_rank(dens):
    """against the definition (min_edge_brute) on stretched blobs with duplicated rows: whole rounds array-equal to
    radius_min_edge_wide, and 3 and 7 segments of the order (6 blocks: the seventh segment is empty) whose merged partials
    equal the whole round, each with populations on the rows of its own blocks only"""
    import torch
    c, r, r2, pairs = reference("min edge")
    n = len(c)
    ct = cuda(c)
    deg = degrees(pairs, n)
    for lab in ("own", "one", "any"):
        comp = graphref.labels(lab, n)
        compt = cuda(comp.astype(np.int32))
        for kind in graphref.RANKS:
            rank = graphref.rank_of(kind, n)
            rankt = cuda(rank.astype(np.int32))
            want = min_edge_brute(pairs, comp, rank, n)
            if lab == "own":
                higher, lower = wg.rank_rule_witnesses(pairs, comp, rank)
                assert higher > 0 and lower > 0, "both branches of the smallest-rank rule"
            best, pops = dens.radius_min_edge_wide_pruned(ct, r2, compt, rankt)
            whole = dens.wide_pruned_info(ct.device)
            assert whole[0] > 0, "the matrix-core kernel did not answer"
            perm = order_of(dens, ct)
            lo, hi = check_counter(c, perm, r, r2, whole)
            assert hi < 16 * 36, "pruning happened"
            assert (u64(best) == want).all(), (lab, kind)
            assert (pops.cpu().numpy().astype(np.int64) == deg).all(), (lab, kind)
            assert ((want != ALL_ONES).any()) == (lab != "one")
            old_b, old_p = dens.radius_min_edge_wide(ct, r2, compt, rankt)
            assert torch.equal(best, old_b) and torch.equal(pops, old_p), (lab, kind)
            for n_seg in (3, 7):
                acc_b = np.full(n, ALL_ONES, dtype=np.uint64)
                acc_p = np.zeros(n, dtype=np.int64)
                tiles = 0
                for g in range(n_seg):
                    b, p = dens.radius_min_edge_wide_pruned(ct, r2, compt, rankt, g, n_seg)
                    info = dens.wide_pruned_info(ct.device)
                    blocks = list(ref.segment_blocks(n, g, n_seg))
                    assert (info[0] > 0) == bool(blocks)
                    check_counter(c, perm, r, r2, info, g, n_seg)
                    mine = np.zeros(n, dtype=bool)
                    for blk in blocks:
                        mine[perm[128 * blk:128 * (blk + 1)]] = True
                    p = p.cpu().numpy().astype(np.int64)
                    assert (p[~mine] == 0).all() and (p[mine] == deg[mine]).all(), (lab, kind, g, n_seg)
                    acc_b = np.minimum(acc_b, u64(b))
                    acc_p += p
                    tiles += info[0]
                assert (acc_b == want).all() and (acc_p == deg).all(), (lab, kind, n_seg)
                assert tiles == whole[0], "the tile counts add up to those of the whole round"


def test_min_edge_across_two_shares_and_radii_that_hold_no_pair(dens):
    c, r, r2, pairs = reference("stretched", 2100, 100)
    n = len(c)
    ct = cuda(c)
    comp = graphref.labels("own", n)
    for kind in ("identity", "random"):
        rank = graphref.rank_of(kind, n)
        higher, lower = wg.rank_rule_witnesses(pairs, comp, rank)
        assert higher > 0 and lower > 0
        compt, rankt = cuda(comp.astype(np.int32)), cuda(rank.astype(np.int32))
        best, pops = dens.radius_min_edge_wide_pruned(ct, r2, compt, rankt)
        info = dens.wide_pruned_info(ct.device)
        assert info[0] > 0
        check_counter(c, order_of(dens, ct), r, r2, info)
        assert (u64(best) == min_edge_brute(pairs, comp, rank, n)).all(), kind
        assert (pops.cpu().numpy().astype(np.int64) == degrees(pairs, n)).all()
    for none in NO_PAIR:
        best, pops = dens.radius_min_edge_wide_pruned(ct, none, compt, rankt)
        assert (u64(best) == ALL_ONES).all() and bool((pops == 1).all()), none
        assert dens.wide_pruned_info(ct.device) == (0, 0, 0)


# ---- the forest ---------------------------------------------------------------------------------------------------------
def forest_cases():
    c, r2 = wg.chain_case(150, 65)
    yield "chain", c, r2
    c, r2, _, _, _ = graphref.bridge(100)
    yield "two cliques and a bridge", c, r2
    c = wideref.blobs(200, 100)
    yield "complete", c, 1.0e6
    yield "empty", c, 1.0e-6
    yield "stretched blobs in two shares", reference("stretched", 2100, 100)[0], reference("stretched", 2100, 100)[2]


def test_forest_against_the_contract(dens, probe):
    for name, c, r2 in forest_cases():
        n = len(c)
        pairs = reference("stretched", 2100, 100)[3] if n == 2100 else brute_pairs(probe, c, r2)
        for kind in ("random", "reversed"):
            rank = graphref.rank_of(kind, n)
            edges, rounds = dens.radius_forest_wide_pruned(c, r2, rank)
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
        edges, rounds = dens.radius_forest_wide_pruned(c, 2.0, np.arange(n, dtype=np.uint32))
        assert edges.shape == (max(n - 1, 0), 2) and rounds == (2 if n == 2 else 0)
        if n == 2:
            assert sorted(edges[0].tolist()) == [0, 1]
            edges, rounds = dens.radius_forest_wide_pruned(c, 1.0, np.arange(n, dtype=np.uint32))   # (d2 = 1 is not < 1)
            assert len(edges) == 0 and rounds == 1
    with pytest.raises(Exception, match="permutation"):
        dens.radius_forest_wide_pruned(np.zeros((3, 100), dtype=np.float32), 1.0, np.array([0, 1, 1], dtype=np.uint32))


def test_forest_has_the_edges_and_rounds_of_the_unpruned_call(dens):
    c, r, r2, pairs = reference("stretched", 1500, 100)
    n = len(c)
    rank = graphref.rank_of("random", n)
    edges, rounds = dens.radius_forest_wide_pruned(c, r2, rank)
    old, old_rounds = dens.radius_forest_wide(c, r2, rank)
    assert len(edges) > 0 and rounds > 1
    check_forest(n, pairs, rank, edges, rounds)
    assert np.array_equal(np.sort(keys(edges, n)), np.sort(keys(old, n))) and rounds == old_rounds


# ---- flagged data -------------------------------------------------------------------------------------------------------
def test_flagged_data_is_answered_by_the_direct_kernels(dens):
    import torch
    c = wg.with_non_finite(ref.stretched(500, 100))
    r2 = wgp.stretched_radius(100)[1]
    n = len(c)
    ct = cuda(c)
    pairs, pops = dens.radius_pairs_wide_pruned(ct, r2)
    assert dens.wide_pruned_info(ct.device) == (0, 0, 0)
    old_pairs, old_pops = dens.radius_pairs_wide(ct, r2)
    assert len(pairs) > 0 and torch.equal(pops, old_pops)
    assert np.array_equal(np.sort(keys(pairs.cpu().numpy(), n)), np.sort(keys(old_pairs.cpu().numpy(), n)))
    assert bool((pops[list(wg.FLAGGED_ROWS)] == 1).all())
    count, part, _, info = raw_pairs(dens, ct, r2, len(pairs) // 3, rows=len(pairs))
    assert count == len(pairs) and info == (0, 0, 0) and (part[len(pairs) // 3:] == -1).all()
    comp, rank = cuda(graphref.labels("any", n).astype(np.int32)), cuda(graphref.rank_of("random", n).astype(np.int32))
    for seg, n_seg in ((0, 0), (1, 3)):   # (a segment: the reference's row block, as the unpruned call answers it)
        best, p = dens.radius_min_edge_wide_pruned(ct, r2, comp, rank, seg, n_seg)
        assert dens.wide_pruned_info(ct.device) == (0, 0, 0)
        old_best, old_p = dens.radius_min_edge_wide(ct, r2, comp, rank, seg, n_seg)
        assert torch.equal(best, old_best) and torch.equal(p, old_p)
    assert (u64(best) != ALL_ONES).any()
    edges, rounds = dens.radius_forest_wide_pruned(c, r2, graphref.rank_of("random", n))
    old, old_rounds = dens.radius_forest_wide(c, r2, graphref.rank_of("random", n))
    assert np.array_equal(np.sort(keys(edges, n)), np.sort(keys(old, n))) and rounds == old_rounds
    # ... and the next call on clean data in the same workspace runs on the matrix cores again
    c, r, r2, want = reference("blobs", 200, 100)
    count, _, _, info = raw_pairs(dens, cuda(c), r2, 0)
    assert count == len(want) and info[0] > 0


# ---- the cap on the exact path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols", [65, 256])
def test_at_most_one_percent_of_the_evaluated_pairs_reach_the_exact_path(dens, n_cols):
    c, r, r2 = wg.blob_case(1500, n_cols)
    ct = cuda(c)
    count, _, _, (tiles, mfmas, exact) = raw_pairs(dens, ct, r2, 0)
    print(f"D={n_cols} pairs: {count} pairs, {tiles} tile pairs, {mfmas} MFMAs, {exact} exact pairs = "
          f"{100.0 * exact / (1024 * max(tiles, 1)):.4f} % of the evaluated pairs")
    assert tiles > 0 and exact <= 0.01 * 1024 * tiles
    comp, rank = cuda(graphref.labels("any", 1500).astype(np.int32)), cuda(graphref.rank_of("random", 1500).astype(np.int32))
    dens.radius_min_edge_wide_pruned(ct, r2, comp, rank)
    tiles, mfmas, exact = dens.wide_pruned_info(ct.device)
    print(f"D={n_cols} min edge: {exact} exact pairs = {100.0 * exact / (1024 * max(tiles, 1)):.4f} % of the evaluated pairs")
    assert tiles > 0 and exact <= 0.01 * 1024 * tiles


# ---- the libraries of the other summation orders ------------------------------------------------------------------------
CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from clustering_amd import capi, density as dens
from oracle.oracle import Probe
import graphref, wideref, widegraphref as wg, widegraphpruneref as wgp, widepruneref as ref
ORDER = sys.argv[2]
assert capi.lib.dc_hip_canon_order().decode() == ORDER
probe = Probe(order=ORDER)
u64 = lambda t: t.cpu().numpy().view(np.uint64)
cases = [wgp.min_edge_case()[:3], (wideref.boundary_case(300, 80)[0], 3.0, np.float32(9.0)),
         (wideref.ties_case(200, 256)[0], None, wg.square(wg.blob_radius(256)))]
for c, r, r2 in cases:
    n = len(c)
    ct = torch.from_numpy(c).cuda()
    want = graphref.brute_pairs(probe, c, r2)
    assert len(want) > 0
    pairs, pops = dens.radius_pairs_wide_pruned(ct, r2)
    tiles = dens.wide_pruned_info(ct.device)[0]
    perm = dens.wide_pruned_order(ct.device).cpu().numpy().astype(np.int64)
    lo, hi = wgp.tile_bounds_r2(c, perm, r2)
    assert tiles > 0 and lo <= tiles <= hi, (c.shape, "the pruning check")
    got = graphref.keys(pairs.cpu().numpy(), n)
    assert len(np.unique(got)) == len(got) and np.array_equal(np.sort(got), graphref.keys(want, n)), (c.shape, "pairs")
    assert (pops.cpu().numpy().astype(np.int64) == graphref.degrees(want, n)).all(), (c.shape, "pops")
    for lab in ("own", "any"):
        comp, rank = graphref.labels(lab, n), graphref.rank_of("random", n)
        best, pops = dens.radius_min_edge_wide_pruned(ct, r2, torch.from_numpy(comp.astype(np.int32)).cuda(),
                                                      torch.from_numpy(rank.astype(np.int32)).cuda())
        assert dens.wide_pruned_info(ct.device)[0] > 0
        assert (u64(best) == graphref.min_edge_brute(want, comp, rank, n)).all(), (c.shape, lab, "best")
        assert (pops.cpu().numpy().astype(np.int64) == graphref.degrees(want, n)).all(), (c.shape, lab, "pops")
    rank = graphref.rank_of("bit-reversed", n)
    edges, rounds = dens.radius_forest_wide_pruned(c, r2, rank)
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
