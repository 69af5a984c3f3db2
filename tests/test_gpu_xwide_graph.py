"""GPU: the radius graph on the matrix-core sweeps of 257..1024 columns, unpruned and pruned (density.radius_pairs_xwide[_pruned],
radius_min_edge_xwide[_pruned], radius_forest_xwide[_pruned]), against brute force over the probe's
canonical d2 matrix (tests/graphref.py) and the oracle's populations.  Every finite case with pairs first asserts that the
matrix-core kernel answered (tiles > 0); every pruned pair call is held to the pruning check, a condition on the counter:
with the block boxes formed in float64 from the device's own order (xwide_pruned_order), 16 #{gap^2 < r2} <= tiles <=
16 #{gap^2 < 1.001 r2}.  Cases: tests/xwidegraphref.py (premises: tests/test_xwide_graph_cases.py, on the CPU).
No referee runs on the GPU, and no call of the 1..64-column graph path is made here."""
import functools

import numpy as np
import pytest

import graphref
import widepruneref as pr
import xwidegraphref as xg
import xwidepruneref as xp
from graphref import ALL_ONES, brute_pairs, check_forest, components, degrees, keys, min_edge_brute

pytestmark = pytest.mark.gpu
FORMS = ("plain", "pruned")
NO_PAIR = (float("nan"), 0.0, -0.0, -1.0, -float("inf"))


@pytest.fixture(scope="module")
def dens():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from clustering_amd import density
    return density


class Form:
    """the three calls of one form, its raw pair call, its counters"""

    def __init__(self, dens, form):
        p = form == "pruned"
        self.pruned, self.dens = p, dens
        self.kind = "xwide_pruned" if p else "xwide"
        self.pairs = dens.radius_pairs_xwide_pruned if p else dens.radius_pairs_xwide
        self.min_edge = dens.radius_min_edge_xwide_pruned if p else dens.radius_min_edge_xwide
        self.forest = dens.radius_forest_xwide_pruned if p else dens.radius_forest_xwide
        self.info = dens.xwide_pruned_info if p else dens.xwide_sweep_info
        self.c_pairs = "dc_hip_radius_pairs_xwide_pruned_dev" if p else "dc_hip_radius_pairs_xwide_dev"

    def raw_pairs(self, ct, r2, capacity, rows=None):
        """one C call with a buffer of `rows` pairs (default: capacity) prefilled with -1, of which the library is told
        `capacity` -> (count, pairs int32 numpy [rows, 2] or None, pops, counters)"""
        import torch
        from clustering_amd import capi
        dens = self.dens
        n, d = ct.shape
        rows = capacity if rows is None else rows
        assert rows >= capacity
        pops = torch.full((n,), -7, dtype=torch.int32, device=ct.device)
        count = torch.full((1,), -7, dtype=torch.int64, device=ct.device)
        pairs = torch.full((rows, 2), -1, dtype=torch.int32, device=ct.device) if rows else None
        with torch.cuda.device(ct.device):
            ws, ws_bytes = dens._get(self.kind, ct.device, n, d, 1)
            rc = getattr(capi.lib, self.c_pairs)(dens._dev(ct), n, d, float(r2), dens._dev(pops),
                                                dens._dev(pairs) if pairs is not None else None, capacity, dens._dev(count),
                                                ws, ws_bytes, dens._stream_ptr())
        capi.check(rc, self.c_pairs)
        torch.cuda.synchronize()
        return int(count.item()), (pairs.cpu().numpy() if pairs is not None else None), pops.cpu().numpy(), self.info(ct.device)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def i32(a):
    return cuda(np.asarray(a).astype(np.int32))


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def order_of(dens, ct):
    perm = dens.xwide_pruned_order(ct.device).cpu().numpy().astype(np.int64)
    assert sorted(perm.tolist()) == list(range(len(ct))), "the order is a permutation of the rows"
    return perm


@functools.lru_cache(maxsize=None)
def reference(case, *shape):
    """(coords, r, r2, brute-force pairs): computed once per case and shared by the tests that need it"""
    from oracle.oracle import Probe, build
    build()
    if case == "stretched":
        c, r, r2 = xg.stretched_case(*shape)
    elif case == "blobs":
        c, r, r2 = xg.blob_case(*shape)
    elif case == "boundary":
        c, r, r2, _ = xg.boundary_case()
    elif case == "small radius":
        c, r, r2, _ = xg.small_radius_case()
    else:
        assert case == "min edge"
        c, r, r2, _ = xg.min_edge_case()
    return c, r, r2, brute_pairs(Probe(), c, r2)


def check_counter(f, c, perm, r2, info):
    """the counters of a whole pair or min-edge call of form f -> (lower, upper) of the tile counter"""
    n_cols = c.shape[1]
    if f.pruned:
        lo, hi = xg.tile_bounds_r2(c, perm, r2)
    else:
        lo = hi = xg.all_tiles(len(c))
    print(f"{'pruned' if f.pruned else 'plain'} {c.shape} r2={float(r2):.6g}: tiles {info[0]} in [{lo}, {hi}], "
          f"all {xg.all_tiles(len(c))}, exact pairs {info[2]}")
    assert lo <= info[0] <= hi, "the pruning check" if f.pruned else "every tile pair"
    assert info[1] == info[0] * xp.mfmas_per_tile_pair(n_cols)
    return lo, hi


def check_pair_list(dens, oracle, c, r, r2, want, forms=FORMS):
    """list, populations, count and counters of both forms against the referees -> {form: (counters, bounds)}, order"""
    n = len(c)
    ct = cuda(c)
    out, perm, sets = {}, None, {}
    deg = degrees(want, n)
    if r is not None:
        assert (deg.astype(np.uint64) == oracle.populations(c, [r])[0]).all(), "degrees + 1 == the oracle's populations"
    for form in forms:
        f = Form(dens, form)
        pairs, pops = f.pairs(ct, r2)
        info = f.info(ct.device)
        assert info[0] > 0 and info[1] > 0, "the matrix-core kernel did not answer"
        if f.pruned:
            perm = order_of(dens, ct)
        bounds = check_counter(f, c, perm, r2, info)
        pairs = pairs.cpu().numpy()
        got = keys(pairs, n)
        assert len(np.unique(got)) == len(got), "a pair was listed twice"
        assert np.array_equal(np.sort(got), keys(want, n)), form
        assert (pairs[:, 0] != pairs[:, 1]).all() and ((pairs >= 0) & (pairs < n)).all()
        if not f.pruned:
            assert (pairs[:, 0] < pairs[:, 1]).all(), "the unpruned list: i < j"
        assert (pops.cpu().numpy().astype(np.int64) == deg).all(), form
        count, none, pops_c, info_c = f.raw_pairs(ct, r2, 0)
        assert count == len(want) and none is None, "d_count is exact with capacity 0"
        assert (pops_c.astype(np.int64) == deg).all() and info_c[:2] == info[:2]
        out[form], sets[form] = (info, bounds), np.sort(got)
    if len(forms) == 2:
        assert np.array_equal(sets["plain"], sets["pruned"]), "pruned set == unpruned set"
    return out, perm


# ---- the pair list ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols", xg.COLS)
def test_pairs_of_300_rows_at_every_column_count(dens, oracle, n_cols):
    c, r, r2, want = reference("stretched", 300, n_cols)
    assert len(want) > 0
    check_pair_list(dens, oracle, c, r, r2, want)


@pytest.mark.parametrize("n_cols", xg.TABLE_COLS)   # (the full cross product with COLS is too long: the table's widths)
@pytest.mark.parametrize("n_rows", xg.STRETCHED_ROWS)
def test_pairs_of_the_stretched_blobs_with_block_pairs_dropped(dens, oracle, n_rows, n_cols):
    c, r, r2, want = reference("stretched", n_rows, n_cols)
    assert len(want) > 0
    out, perm = check_pair_list(dens, oracle, c, r, r2, want)
    (info, (lo, hi)), (plain, _) = out["pruned"], out["plain"]
    assert hi < xg.all_tiles(n_rows) and info[0] < plain[0] == xg.all_tiles(n_rows), "below the unpruned count"
    assert lo >= 16 * pr.n_blocks(n_rows), "every block meets itself"
    assert not np.array_equal(perm, np.arange(n_rows)), "the order is not the identity"


@pytest.mark.parametrize("n_rows", [1, 2, 129])
def test_pairs_of_a_few_rows(dens, oracle, n_rows):
    c, r, r2, want = reference("stretched", n_rows, 300)
    out, _ = check_pair_list(dens, oracle, c, r, r2, want)
    assert out["plain"][0][1] == 57 * out["plain"][0][0], "57 MFMAs per tile pair at 300 columns"


def test_pairs_on_and_one_ulp_to_either_side_of_the_radius(dens, oracle):
    c, r, r2, want = reference("boundary")
    groups = xg.boundary_case()[3]
    out, _ = check_pair_list(dens, oracle, c, r, r2, want)
    n = len(c)
    for form in FORMS:
        assert out[form][0][2] > 0, "pairs exactly on a radius can only be decided by the exact path"
        pairs, _ = Form(dens, form).pairs(cuda(c), r2)
        got = set(keys(pairs.cpu().numpy(), n).tolist())
        for a, b, cc, d in groups:
            assert int(keys([[a, b]], n)[0]) not in got, "the pair on the radius"
            assert int(keys([[a, cc]], n)[0]) not in got, "the pair one ulp outside"
            assert int(keys([[a, d]], n)[0]) in got, "the pair one ulp inside"


def test_units_without_a_survivor_still_add_the_frames_own_one(dens, oracle):
    c, r, r2, want = reference("small radius")
    dups = xg.small_radius_case()[3]
    n = len(c)
    assert np.array_equal(np.sort(keys(want, n)), np.sort(keys(dups, n))), "the duplicates and nothing else"
    out, perm = check_pair_list(dens, oracle, c, r, r2, want)
    empty, units = pr.empty_units(c, perm, float(r2))
    print(f"{empty} of {units} (query block, share) units without a survivor")
    assert units == 8 * 65 and empty > 0, "the premise, from the device's order"
    assert out["pruned"][0][0] < out["plain"][0][0]


def test_the_complete_graph_and_radii_that_hold_no_pair(dens, oracle, probe):
    c = xg.blob_case(300, 257)[0]
    n = len(c)
    ii, jj = np.triu_indices(n, 1)
    everything = np.stack([ii, jj], axis=1).astype(np.int64)
    d2 = probe.pairwise_d2(c)
    least = float(d2[~np.eye(n, dtype=bool)].min())
    assert 0.0 < least < 1.0e6
    for r2 in (1.0e6, 3.0e38, float("inf")):
        out, _ = check_pair_list(dens, oracle, c, None, r2, everything)
        assert out["pruned"][0][0] == out["plain"][0][0] == 16 * 9
    ct = cuda(c)
    for form in FORMS:
        f = Form(dens, form)
        for r2 in NO_PAIR:
            count, part, pops, info = f.raw_pairs(ct, r2, 16)
            assert count == 0 and (part == -1).all() and (pops == 1).all(), (form, r2)
            if f.pruned:
                assert info == (0, 0, 0), "no block pair can hold a pair: nothing is evaluated"
            pairs, pops = f.pairs(ct, r2)
            assert pairs.shape == (0, 2) and bool((pops == 1).all())
        # below the least d2 of the data: the sweep runs and finds nothing (strict <: the closest pair itself is outside)
        count, part, pops, info = f.raw_pairs(ct, least, 16)
        assert count == 0 and (part == -1).all() and (pops == 1).all() and info[0] > 0, form
        count, _, _, _ = f.raw_pairs(ct, np.nextafter(np.float32(least), np.float32(np.inf)), 0)
        assert count == int((d2[ii, jj] == np.float32(least)).sum()) > 0, "one float above it: the closest pairs"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", [("stretched", 700, 1024), ("boundary",)])
def test_capacity(dens, case, form):
    """capacities count - 1, count / 2 and 1: the full count, exactly `capacity` distinct valid pairs, the rest of a prefilled
    buffer untouched; and exactly the count"""
    c, r, r2, want = reference(*case)
    n, total = len(c), len(want)
    assert total >= 4
    ct = cuda(c)
    f = Form(dens, form)
    want_keys = keys(want, n)
    deg = degrees(want, n)
    for cap in (total - 1, total // 2, 1):
        count, part, pops, info = f.raw_pairs(ct, r2, cap, rows=cap + 64)
        assert count == total and info[0] > 0, "the full count, whatever the capacity"
        assert (part[cap:] == -1).all(), "nothing is written beyond the capacity"
        assert ((part[:cap] >= 0) & (part[:cap] < n)).all() and (part[:cap, 0] != part[:cap, 1]).all()
        assert np.isin(keys(part[:cap], n), want_keys).all() and len(np.unique(keys(part[:cap], n))) == cap
        assert (pops.astype(np.int64) == deg).all()
    count, part, _, _ = f.raw_pairs(ct, r2, total, rows=total + 64)
    assert count == total and (part[total:] == -1).all()
    assert np.array_equal(np.sort(keys(part[:total], n)), want_keys)


# ---- the cap on the exact path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols", xg.TABLE_COLS)
def test_the_exact_path_of_the_stretched_case_stays_inside_its_bound(dens, n_cols):
    """the bound derived for the one-radius population call on the same data (xwidepruneref.stretched_band_bound), which is
    this sweep"""
    c, r, r2, want = reference("stretched", 1500, n_cols)
    bound = xp.stretched_band_bound(n_cols)
    ct = cuda(c)
    comp, rank = i32(graphref.labels("any", 1500)), i32(graphref.rank_of("random", 1500))
    for form in FORMS:
        f = Form(dens, form)
        count, _, _, (tiles, mfmas, exact) = f.raw_pairs(ct, r2, 0)
        print(f"D={n_cols} {form} pairs: {count} pairs, {tiles} tile pairs, {exact} exact pairs = "
              f"{100.0 * exact / (1024 * max(tiles, 1)):.4f} % of the evaluated pairs, bound {bound}")
        assert count == len(want) and tiles > 0 and exact <= bound
        f.min_edge(ct, r2, comp, rank)
        tiles, mfmas, exact = f.info(ct.device)
        print(f"D={n_cols} {form} min edge: {exact} exact pairs, bound {bound}")
        assert tiles > 0 and exact <= bound


# ---- one Boruvka round --------------------------------------------------------------------------------------------------
def rows_brute(pairs, comp, rank, n, lo, hi):
    """d_best of the queries lo .. hi - 1 of one round: per component id the smallest key over the (query, partner) meetings
    whose query lies in the row block"""
    both = np.concatenate([pairs, pairs[:, ::-1]])
    both = both[(both[:, 0] >= lo) & (both[:, 0] < hi)]
    want = np.full(n, ALL_ONES, dtype=np.uint64)
    q, p = both[:, 0], both[:, 1]
    cross = comp[q] != comp[p]
    q, p = q[cross], p[cross]
    key = (np.maximum(rank[q], rank[p]).astype(np.uint64) << np.uint64(32)) | np.minimum(rank[q], rank[p]).astype(np.uint64)
    np.minimum.at(want, comp[q], key)
    return want


@pytest.mark.parametrize("lab", ("own", "one", "any"))
def test_min_edge_round_for_every_labelling_and_rank(dens, lab):
    """against the definition (min_edge_brute): whole rounds of both forms, and 1, 2, 3 and 7 segments -- of the order
    (pruned; 6 blocks: the seventh segment is empty) or of the rows (unpruned: the reference's row block) -- whose partials
    merge by minimum / sum into the whole round"""
    import torch
    c, r, r2, pairs = reference("min edge")
    n = len(c)
    ct = cuda(c)
    deg = degrees(pairs, n)
    comp = graphref.labels(lab, n)
    compt = i32(comp)
    for kind in graphref.RANKS:
        rank = graphref.rank_of(kind, n)
        rankt = i32(rank)
        want = min_edge_brute(pairs, comp, rank, n)
        assert ((want != ALL_ONES).any()) == (lab != "one")
        whole = {}
        for form in FORMS:
            f = Form(dens, form)
            best, pops = f.min_edge(ct, r2, compt, rankt)
            info = f.info(ct.device)
            assert info[0] > 0, "the matrix-core kernel did not answer"
            perm = order_of(dens, ct) if f.pruned else None
            lo, hi = check_counter(f, c, perm, r2, info)
            assert (u64(best) == want).all(), (form, lab, kind)
            assert (pops.cpu().numpy().astype(np.int64) == deg).all(), (form, lab, kind)
            whole[form] = (best, pops, info, perm)
            if f.pruned:
                assert hi < 16 * 36, "pruning happened"
        assert torch.equal(whole["plain"][0], whole["pruned"][0]) and torch.equal(whole["plain"][1], whole["pruned"][1])
        for form in FORMS:
            f = Form(dens, form)
            perm = whole[form][3]
            for n_seg in (1, 2, 3, 7):
                acc_b = np.full(n, ALL_ONES, dtype=np.uint64)
                acc_p = np.zeros(n, dtype=np.int64)
                tiles = 0
                for g in range(n_seg):
                    b, p = f.min_edge(ct, r2, compt, rankt, g, n_seg)
                    info = f.info(ct.device)
                    p = p.cpu().numpy().astype(np.int64)
                    mine = np.zeros(n, dtype=bool)
                    if f.pruned:
                        blocks = list(pr.segment_blocks(n, g, n_seg))
                        assert (info[0] > 0) == bool(blocks), (g, n_seg)
                        t_lo, t_hi = xg.tile_bounds_r2(c, perm, r2, g, n_seg)
                        assert t_lo <= info[0] <= t_hi, "the pruning check of a segment"
                        for blk in blocks:
                            mine[perm[128 * blk:128 * (blk + 1)]] = True
                    else:
                        lo_row = g * (n // n_seg)
                        hi_row = n if g == n_seg - 1 else lo_row + n // n_seg
                        mine[lo_row:hi_row] = True
                        assert (u64(b) == rows_brute(pairs, comp, rank, n, lo_row, hi_row)).all(), "the reference's row block"
                    assert (p[~mine] == 0).all() and (p[mine] == deg[mine]).all(), (form, lab, kind, g, n_seg)
                    acc_b = np.minimum(acc_b, u64(b))
                    acc_p += p
                    tiles += info[0]
                assert (acc_b == want).all() and (acc_p == deg).all(), (form, lab, kind, n_seg)
                if f.pruned:
                    assert tiles == whole[form][2][0], "the tile counts add up to those of the whole round"


@pytest.mark.parametrize("form", FORMS)
def test_min_edge_across_two_shares_and_radii_that_hold_no_pair(dens, form):
    c, r, r2, pairs = reference("stretched", 2100, 257)
    n = len(c)
    assert pr.shares(pr.n_blocks(n)) == 2
    ct = cuda(c)
    f = Form(dens, form)
    comp = graphref.labels("own", n)
    compt = i32(comp)
    for kind in ("identity", "random"):
        rank = graphref.rank_of(kind, n)
        rankt = i32(rank)
        best, pops = f.min_edge(ct, r2, compt, rankt)
        info = f.info(ct.device)
        assert info[0] > 0
        check_counter(f, c, order_of(dens, ct) if f.pruned else None, r2, info)
        assert (u64(best) == min_edge_brute(pairs, comp, rank, n)).all(), kind
        assert (pops.cpu().numpy().astype(np.int64) == degrees(pairs, n)).all()
    for none in NO_PAIR:
        best, pops = f.min_edge(ct, none, compt, rankt)
        assert (u64(best) == ALL_ONES).all() and bool((pops == 1).all()), none
        if f.pruned:
            assert f.info(ct.device) == (0, 0, 0)


# ---- the forest ---------------------------------------------------------------------------------------------------------
def forest_cases(n_cols):
    yield "chain", xg.embedded(graphref.chain(150), n_cols), 2.0
    c, r2, _ = graphref.star(8)
    yield "star", xg.embedded(c, n_cols), r2
    c, r2, _, _, _ = graphref.bridge(4)
    yield "two cliques and a bridge", xg.embedded(c, n_cols), r2
    yield "chain with isolated rows", xg.embedded(graphref.with_isolated(graphref.chain(150)), n_cols), 2.0


@pytest.mark.parametrize("n_cols", [257, 1024])
def test_forest_against_the_contract(dens, probe, n_cols):
    for name, c, r2 in forest_cases(n_cols):
        n = len(c)
        pairs = brute_pairs(probe, c, r2)
        n_comp = len(np.unique(components(n, pairs)))
        for kind in ("random", "reversed"):
            rank = graphref.rank_of(kind, n)
            got = {}
            for form in FORMS:
                edges, rounds = Form(dens, form).forest(c, r2, rank)
                assert check_forest(n, pairs, rank, edges, rounds) == n_comp, (name, form, kind)
                got[form] = (np.sort(keys(edges, n)), rounds)
            assert np.array_equal(got["plain"][0], got["pruned"][0]) and got["plain"][1] == got["pruned"][1], \
                "the pruned forest has the edges and rounds of the unpruned one"
        assert (len(edges) == n - 1) == (name != "chain with isolated rows"), name
        if name == "chain with isolated rows":
            assert n_comp == 8 and len(edges) == n - 8


@pytest.mark.parametrize("form", FORMS)
def test_forest_of_no_one_and_two_rows(dens, form):
    forest = Form(dens, form).forest
    for n in (0, 1, 2):
        c = np.zeros((n, 300), dtype=np.float32)
        if n == 2:
            c[1, 299] = 1.0
        edges, rounds = forest(c, 2.0, np.arange(n, dtype=np.uint32))
        assert edges.shape == (max(n - 1, 0), 2) and rounds == (2 if n == 2 else 0)
        if n == 2:
            assert sorted(edges[0].tolist()) == [0, 1]
            edges, rounds = forest(c, 1.0, np.arange(n, dtype=np.uint32))   # (d2 = 1 is not < 1)
            assert len(edges) == 0 and rounds == 1
    with pytest.raises(Exception, match="permutation"):
        forest(np.zeros((3, 300), dtype=np.float32), 1.0, np.array([0, 1, 1], dtype=np.uint32))


def test_forest_of_the_stretched_blobs_has_the_edges_and_rounds_of_the_unpruned_call(dens):
    c, r, r2, pairs = reference("stretched", 1500, 257)
    n = len(c)
    rank = graphref.rank_of("random", n)
    edges, rounds = dens.radius_forest_xwide_pruned(c, r2, rank)
    old, old_rounds = dens.radius_forest_xwide(c, r2, rank)
    assert len(edges) > 0 and rounds > 1
    check_forest(n, pairs, rank, edges, rounds)
    assert np.array_equal(np.sort(keys(edges, n)), np.sort(keys(old, n))) and rounds == old_rounds


# ---- flagged data -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols", xg.FLAGGED_COLS)   # (the generic direct kernel | beyond 400 columns the column-chunked one)
@pytest.mark.parametrize("flaw", xg.FLAWS)
def test_flagged_data_is_answered_by_the_direct_kernels(dens, probe, flaw, n_cols):
    clean, r, r2, _ = reference("stretched", 300, n_cols)
    c = xg.flawed(clean, flaw)
    n = len(c)
    want = brute_pairs(probe, c, r2)
    deg = degrees(want, n)
    assert len(want) > 0
    ct = cuda(c)
    comp, rank = graphref.labels("any", n), graphref.rank_of("random", n)
    compt, rankt = i32(comp), i32(rank)
    best_want = min_edge_brute(want, comp, rank, n)
    n_comp = len(np.unique(components(n, want)))
    for form in FORMS:
        f = Form(dens, form)
        pairs, pops = f.pairs(ct, r2)
        assert f.info(ct.device) == (0, 0, 0), "counters (0, 0, 0)"
        pairs = pairs.cpu().numpy()
        assert np.array_equal(np.sort(keys(pairs, n)), keys(want, n)) and len(np.unique(keys(pairs, n))) == len(pairs)
        assert (pops.cpu().numpy().astype(np.int64) == deg).all()
        cap = len(want) // 3
        count, part, _, info = f.raw_pairs(ct, r2, cap, rows=len(want))
        assert count == len(want) and info == (0, 0, 0) and (part[cap:] == -1).all()
        assert len(np.unique(keys(part[:cap], n))) == cap and np.isin(keys(part[:cap], n), keys(want, n)).all()
        best, p = f.min_edge(ct, r2, compt, rankt)
        assert f.info(ct.device) == (0, 0, 0)
        assert (u64(best) == best_want).all() and (p.cpu().numpy().astype(np.int64) == deg).all()
        acc_b, acc_p = np.full(n, ALL_ONES, dtype=np.uint64), np.zeros(n, dtype=np.int64)
        for g in range(3):   # (a segment of either form on flagged data: the reference's row block)
            b, p = f.min_edge(ct, r2, compt, rankt, g, 3)
            assert f.info(ct.device) == (0, 0, 0)
            assert (u64(b) == rows_brute(want, comp, rank, n, g * 100, (g + 1) * 100)).all(), (form, g)
            acc_b, acc_p = np.minimum(acc_b, u64(b)), acc_p + p.cpu().numpy().astype(np.int64)
        assert (acc_b == best_want).all() and (acc_p == deg).all()
        edges, rounds = f.forest(c, r2, rank)
        assert check_forest(n, want, rank, edges, rounds) == n_comp
        # ... and the next call on clean data in the same workspace runs on the matrix cores again
        count, _, _, info = f.raw_pairs(cuda(clean), r2, 0)
        assert count == len(reference("stretched", 300, n_cols)[3]) and info[0] > 0


# ---- transforms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols", [257, 1024])
def test_lattice_data_scaled_and_shifted(dens, probe, n_cols):
    """graphref.TRANSFORMS: exact powers of two and an integer shift keep every d2 of the lattice an exact multiple of what
    it was, so the pair set of a tie radius -- pairs ON it outside, pairs one float below the next radius inside -- stays"""
    base = graphref.lattice(300, n_cols, seed=n_cols)
    n = len(base)
    d2 = probe.pairwise_d2(base)
    radii = graphref.tie_radii(d2, graphref.level_of(d2, 2))
    comp, rank = graphref.labels("any", n), graphref.rank_of("bit-reversed", n)
    for r2 in radii[1:]:
        plain_set = keys(graphref.pairs_of(d2, r2), n)
        assert len(plain_set) > 0
        for name, scale, shift in graphref.TRANSFORMS:
            c, r2_t = graphref.transformed(base, r2, scale, shift)
            want = brute_pairs(probe, c, r2_t)
            assert np.array_equal(keys(want, n), plain_set), (name, "the premise: the transform keeps the pair set")
            ct = cuda(c)
            for form in FORMS:
                f = Form(dens, form)
                pairs, pops = f.pairs(ct, float(r2_t))
                got = keys(pairs.cpu().numpy(), n)
                assert len(np.unique(got)) == len(got) and np.array_equal(np.sort(got), plain_set), (name, form)
                assert (pops.cpu().numpy().astype(np.int64) == degrees(want, n)).all(), (name, form)
                best, _ = f.min_edge(ct, float(r2_t), i32(comp), i32(rank))
                assert (u64(best) == min_edge_brute(want, comp, rank, n)).all(), (name, form)
