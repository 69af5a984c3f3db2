"""GPU (-m gpu): the matrix-core radius graph -- the pair list (dc_hip_radius_pairs_dev / dc_hip_radius_pairs), one
Boruvka round (dc_hip_radius_min_edge[_segment]_dev) and the forest (dc_hip_radius_forest, Session.radius_forest,
distributed.ShardedForest) -- at its edges, against the probe's canonical d2 matrix (tests/graphref.py) and never
against another GPU kernel.  The pruned population sweep runs these with a sink (kSinkPairs / kSinkMinEdge,
dc_mfma_kernels.hpp) that no population test looks at:

 1. a NaN r2 (no pair: d2 < NaN holds for none), next to 0, -1, -0.0, a subnormal, 1e30 and +inf;
 2. pad positions of the spatial order must never come out as a partner: no frame id >= n_rows in the list, no rank
    0xFFFFFFFF in d_best -- with ONE component over all rows d_best is all ones everywhere;
 3. a pair buffer shorter than the list: the full count, exactly `capacity` true pairs, nothing behind the buffer;
 4. ties: a pair with d2 == r2 is outside, a pair one float below r2 is inside (pairs the accumulator alone decides
    "inside" skip the exact re-check);
 5. the forest contract at EVERY rank threshold, on chains, stars, cliques, bridges and isolated frames.

The data are integer lattices (exact d2 in every summation order), also scaled by 2^-40 / 2^20 and shifted by 1024.
Every device-pointer call on finite data of <= 64 columns also reads header word 1 of the self workspace: 0 -- the
matrix-core kernel answered, not the direct kernel behind the statistics flag; flagged data asserts the opposite.  (The
host-pointer forms keep their workspace inside a session; the sharded loop runs the same rounds on the checked one.)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import graphref as G
from graphref import ALL_ONES, INF, NAN, F32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = [1, 3, 10, 30, 33, 64]            # both sides of the register / LDS operand seam and of the MFMA-count steps
SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 257]   # around the 32-row tile and the query group
DC_ERR_INVALID_ARGUMENT = -1
MIN_EDGE_MAX_ROWS = (1 << 24) - 64 * 512  # dc_mfma.hpp kMinEdgeMaxRows = 2^24 - kOrderPadRows


@pytest.fixture(scope="module")
def dens():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from clustering_amd import density
    return density


@pytest.fixture(scope="module")
def probe():
    from clustering_amd import capi
    from oracle.oracle import Probe, build
    build()
    return Probe(capi.CANON_ORDER)


def gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def flag_word(dens, t):
    """header word 1 of the self workspace on t's device: the statistics flag of the last sweep"""
    return int(dens._workspace(t.device).buf[4:8].cpu().numpy().view(np.uint32)[0])


def answered(dens, t, what, flagged=False):
    """after a call on <= 64 columns: the matrix-core kernel answered (word 1 == 0) unless the data are flagged"""
    assert t.shape[1] <= 64
    w = flag_word(dens, t)
    if flagged:
        assert w != 0, (what, "the statistics flag should be set")
    else:
        assert w == 0, (what, "the matrix-core kernel should have answered, flag word", w)


def special_r2(d2, level_index=1):
    """the r2 values of the issue: 0, -1, -0.0, a subnormal, a lattice d2 with its two float neighbours, 1e30, inf, NaN"""
    out = [0.0, -1.0, -0.0, 1e-45, 1e30, INF, NAN]
    off = ~np.eye(len(d2), dtype=bool)
    if len(d2) >= 31 and (d2[off] > 0).any():
        out += list(G.tie_radii(d2, G.level_of(d2, level_index)))
    return out


# ---- the pair list ------------------------------------------------------------------------------------------------------
def check_pairs(dens, d2, ct, r2, what, flagged=False):
    """every check of the issue's pair-list section for one (data, r2) -> the brute-force pairs"""
    n = ct.shape[0]
    want = G.pairs_of(d2, r2)
    want_keys = G.keys(want, n)
    deg = G.degrees(want, n)
    total = len(want)
    if not (F32(r2) > 0):    # negative, zero and NaN r2: no pairs, populations of 1
        assert total == 0 and (deg == 1).all()
    if F32(r2) == F32(INF):
        assert total == n * (n - 1) // 2
    pairs, pops = dens.radius_pairs(ct, r2)
    answered(dens, ct, what, flagged)
    p = pairs.cpu().numpy()
    assert p.shape == (total, 2), (what, "pairs listed", len(p), "expected", total)
    assert ((p >= 0) & (p < n)).all(), (what, "a frame id beyond n_rows (a pad position of the order?)", p[(p < 0) | (p >= n)][:4])
    assert (p[:, 0] != p[:, 1]).all(), (what, "a pair of a frame with itself")
    got = G.keys(p, n)
    assert len(np.unique(got)) == len(got), (what, "a pair was listed twice")
    assert np.array_equal(np.sort(got), want_keys), what
    assert (pops.cpu().numpy().astype(np.int64) == deg).all(), (what, "populations")
    # counting only (NULL, 0)
    count, _, pops_c = G.raw_pairs(dens, ct, r2, 0)
    answered(dens, ct, what, flagged)
    assert count == total and (pops_c.astype(np.int64) == deg).all(), (what, "count only", count, total)
    # short buffers: the full count, exactly `capacity` distinct true pairs, nothing behind them.  The buffer is as long
    # as the whole list (+ 64 rows), so that every row the library was not given is a sentinel.
    for cap in sorted({1, total // 3, total - 1}):
        if not 0 < cap < total:
            continue
        count, part, pops_s = G.raw_pairs(dens, ct, r2, cap, rows=total + 64)
        answered(dens, ct, what, flagged)
        assert count == total, (what, "capacity", cap, "count", count)
        assert (part[cap:] == -1).all(), (what, "capacity", cap, "rows behind the buffer were written",
                                          np.flatnonzero((part[cap:] != -1).any(axis=1))[:4] + cap)
        head = part[:cap]
        assert ((head >= 0) & (head < n)).all() and (head[:, 0] != head[:, 1]).all(), (what, "capacity", cap)
        hk = G.keys(head, n)
        assert np.isin(hk, want_keys).all() and len(np.unique(hk)) == cap, (what, "capacity", cap)
        assert (pops_s.astype(np.int64) == deg).all(), (what, "capacity", cap, "populations")
    # the exact-size buffer with sentinels behind it
    if total:
        count, part, _ = G.raw_pairs(dens, ct, r2, total, rows=total + 64)
        assert count == total and (part[total:] == -1).all(), (what, "exact capacity")
        assert np.array_equal(np.sort(G.keys(part[:total], n)), want_keys), (what, "exact capacity")
    return want


@pytest.mark.parametrize("D", DIMS)
def test_pair_list_special_r2_and_ties_across_the_tile(dens, probe, D):
    """points 1, 3 and 4: every r2 of the list (NaN and negative: nothing; inf and 1e30: all n(n-1)/2; the tie level: the
    pairs AT r2 stay out, the pairs one float below r2 are in) at row counts around the 32-row tile, with the short and
    sentinel-padded buffers of check_pairs at each"""
    for n in SIZES:
        c = G.lattice(n, D, seed=100 * D + n)
        d2 = probe.pairwise_d2(c)
        ct = gpu(c)
        for r2 in special_r2(d2):
            check_pairs(dens, d2, ct, r2, (f"lattice n={n} D={D}", "r2", r2))


@pytest.mark.parametrize("D", DIMS)
def test_pair_list_on_scaled_and_shifted_lattices(dens, probe, D):
    """the same on data scaled by 2^-40 and 2^20 (r2 by the square) and shifted by 1024 (exact differences, a Gram form
    that cancels hard): the tie decisions must not move"""
    for n in (65, 257):
        base = G.lattice(n, D, seed=7 * D + n)
        d2_base = probe.pairwise_d2(base)
        for level_index in (0, 2):
            for name, scale, shift in G.TRANSFORMS:
                for r2_base in G.tie_radii(d2_base, G.level_of(d2_base, level_index)):
                    c, r2 = G.transformed(base, r2_base, scale, shift)
                    d2 = probe.pairwise_d2(c)
                    want = check_pairs(dens, d2, gpu(c), r2, (f"{name} n={n} D={D}", "r2", r2))
                    assert np.array_equal(want, G.pairs_of(d2_base, r2_base)), "the transform moved a tie"
        for name, scale, shift in G.TRANSFORMS[1:]:
            c, _ = G.transformed(base, 1.0, scale, shift)
            d2 = probe.pairwise_d2(c)
            for r2 in (0.0, 1e-45, NAN, 1e30, INF):
                check_pairs(dens, d2, gpu(c), r2, (f"{name} n={n} D={D}", "r2", r2))


@pytest.mark.parametrize("D,n", [(1, 3000), (3, 3001), (10, 2500), (33, 2047), (64, 2048)])
def test_pair_list_on_lattice_clusters(dens, probe, D, n):
    """points 2 and 4 where the pruning engages: clusters 64 apart -- components of the order, each padded to whole query
    groups -- at the tie radii, and (n <= 2048) at 1e30 / inf, where every real pair is inside and a pad position must
    still never be listed"""
    c = G.clustered_lattice(n, D, seed=300 + D)
    d2 = probe.pairwise_d2(c)
    ct = gpu(c)
    radii = list(G.tie_radii(d2, G.level_of(d2, 1))) + [NAN, 0.0]
    if n <= 2048:
        radii += [1e30, INF]
    for r2 in radii:
        check_pairs(dens, d2, ct, r2, (f"clusters n={n} D={D}", "r2", r2))


@pytest.mark.parametrize("D", [1, 10, 33, 64])
def test_pair_list_of_duplicates_one_row_and_no_rows(dens, probe, D):
    """all rows the same: the complete graph at any r2 > 0 (every pair in the band at d2 = 0), the empty one at r2 = 0;
    a single row; zero rows"""
    import torch
    for n in (33, 500):
        c = np.full((n, D), 3.0, dtype=np.float32)
        d2 = probe.pairwise_d2(c)
        ct = gpu(c)
        for r2 in (1e-45, 1.0, INF, 0.0, -0.0, NAN, -1.0):
            want = check_pairs(dens, d2, ct, r2, (f"duplicates n={n} D={D}", "r2", r2))
            assert len(want) == (n * (n - 1) // 2 if r2 > 0 else 0)
    one = gpu(np.full((1, D), 2.0, dtype=np.float32))
    for r2 in (0.0, 1.0, INF, NAN):
        check_pairs(dens, np.zeros((1, 1), dtype=np.float32), one, r2, (f"one row D={D}", r2))
    count, _, _ = G.raw_pairs(dens, torch.zeros((0, D), dtype=torch.float32, device="cuda"), 1.0, 0)
    assert count == 0


@pytest.mark.parametrize("D", [3, 33])
def test_pair_list_behind_the_statistics_flag(dens, probe, D):
    """the opposite of the header check: one row beyond the 1e36 norm limit sets word 1, the direct kernel answers, and
    the next call on clean data is answered by the matrix cores again"""
    c = G.lattice(257, D, seed=40 + D)
    bad = c.copy()
    bad[100, 0] = F32(2e18)
    for r2 in (2.0, NAN):
        check_pairs(dens, probe.pairwise_d2(bad), gpu(bad), r2, (f"flagged D={D}", r2), flagged=True)
    check_pairs(dens, probe.pairwise_d2(c), gpu(c), 2.0, (f"clean after the flag D={D}",))


def host_pairs(c, r2, capacity, rows):
    """dc_hip_radius_pairs (host pointers) with a buffer of `rows` pairs prefilled with ~0 -> (count, buffer)"""
    from clustering_amd import capi
    n, d = c.shape
    buf = np.full((max(rows, 1), 2), 0xFFFFFFFF, dtype=np.uint32)
    count = C.c_uint64(0)
    capi.check(capi.lib.dc_hip_radius_pairs(c.ctypes.data_as(C.c_void_p), n, d, float(r2), 0,
                                            buf.ctypes.data_as(C.c_void_p) if capacity else None, capacity,
                                            C.byref(count)), "dc_hip_radius_pairs")
    return int(count.value), buf


@pytest.mark.parametrize("D", [3, 33, 64])
def test_host_pair_list(dens, probe, D):
    """dc_hip_radius_pairs: the same sets, counts and short buffers through the host-pointer form"""
    for n in (0, 1, 33, 257):
        c = G.lattice(n, D, seed=50 + D + n) if n else np.zeros((0, D), dtype=np.float32)
        d2 = probe.pairwise_d2(c) if n else np.zeros((0, 0), dtype=np.float32)
        for r2 in (special_r2(d2) if n else [1.0, NAN]):
            want = G.pairs_of(d2, r2)
            total = len(want)
            what = (f"host n={n} D={D}", "r2", r2)
            count, _ = host_pairs(c, r2, 0, 0)
            assert count == total, what
            for cap in sorted({1, total // 3, total - 1, total}):
                if not 0 < cap <= total:
                    continue
                count, buf = host_pairs(c, r2, cap, total + 64)
                assert count == total, what
                assert (buf[cap:] == 0xFFFFFFFF).all(), (what, "capacity", cap, "rows behind the buffer were written")
                head = buf[:cap].astype(np.int64)
                assert (head < n).all() and (head[:, 0] != head[:, 1]).all(), (what, "capacity", cap)
                hk = G.keys(head, n)
                assert len(np.unique(hk)) == cap and np.isin(hk, G.keys(want, n)).all(), (what, "capacity", cap)


# ---- one Boruvka round --------------------------------------------------------------------------------------------------
def min_edge(dens, ct, r2, comp, rank, segment=0, n_segments=0, what=None, flagged=False):
    best, pops = dens.radius_min_edge(ct, r2, gpu(comp.view(np.int32)), gpu(rank.view(np.int32)), segment, n_segments)
    answered(dens, ct, what, flagged)
    return best.cpu().numpy().view(np.uint64), pops.cpu().numpy().astype(np.int64)


def check_min_edge(dens, d2, ct, r2, comp, rank, what):
    n = ct.shape[0]
    pairs = G.pairs_of(d2, r2)
    want = G.min_edge_brute(pairs, comp, rank, n)
    got, pops = min_edge(dens, ct, r2, comp, rank, what=what)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, "d_best differs at", bad[:4], [hex(int(x)) for x in got[bad[:4]]],
                           [hex(int(x)) for x in want[bad[:4]]])
    assert (pops == G.degrees(pairs, n)).all(), (what, "populations")
    if not (F32(r2) > 0):
        assert (got == ALL_ONES).all() and (pops == 1).all(), what
    return got, pops, pairs


def check_segments(dens, ct, r2, comp, rank, n_seg, whole, pops_whole, what):
    n = ct.shape[0]
    acc_b = np.full(n, ALL_ONES, dtype=np.uint64)
    acc_p = np.zeros(n, dtype=np.int64)
    for g in range(n_seg):
        b, p = min_edge(dens, ct, r2, comp, rank, g, n_seg, what=what + ("segment", g, n_seg))
        acc_b = np.minimum(acc_b, b)
        acc_p += p
    assert (acc_b == whole).all(), what + ("segments", n_seg, "d_best")
    assert (acc_p == pops_whole).all(), what + ("segments", n_seg, "populations")


@pytest.mark.parametrize("D", DIMS)
def test_min_edge_round_special_r2_labels_and_ranks(dens, probe, D):
    """points 1, 2 and 4 for the round: every r2 of the list against min_edge_brute, with every frame its own component,
    one component over all rows (nothing leaves it: all ones everywhere -- a pad position that came out as a partner
    would leave a key with rank 0xFFFFFFFF), and components named by a member that is not their smallest; identity,
    reversed, bit-reversed and random ranks"""
    for n in (1, 2, 33, 65, 257):
        c = G.lattice(n, D, seed=900 + 10 * D + n)
        d2 = probe.pairwise_d2(c)
        ct = gpu(c)
        for r2 in special_r2(d2):
            for lab in ("own", "one", "any"):
                comp = G.labels(lab, n, seed=D)
                for kind in G.RANKS:
                    got, _, _ = check_min_edge(dens, d2, ct, r2, comp, G.rank_of(kind, n, D),
                                               (f"n={n} D={D}", "r2", r2, lab, kind))
                    if lab == "one":
                        assert (got == ALL_ONES).all()


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("n", [33, 1000])
def test_one_component_over_all_rows_meets_only_pad_positions(dens, probe, D, n):
    """point 2 at its sharpest: r2 = inf (and 1e30), ONE component, n_rows no multiple of 32 -- every real partner is in
    the query's own component, so the only positions that could yield a key are the pads of the order: d_best must be
    all ones everywhere.  With every frame its own component the same sweep gives every component a key."""
    c = G.clustered_lattice(n, D, seed=60 + D) if n > 33 else G.lattice(n, D, seed=60 + D)
    d2 = probe.pairwise_d2(c)
    ct = gpu(c)
    assert n % 32 != 0
    for r2 in (INF, 1e30):
        for kind in G.RANKS:
            rank = G.rank_of(kind, n, D)
            for comp in (G.labels("one", n), np.full(n, 0, dtype=np.uint32), np.full(n, n // 2, dtype=np.uint32)):
                got, pops, _ = check_min_edge(dens, d2, ct, r2, comp, rank, (f"one component n={n} D={D}", r2, kind))
                assert (got == ALL_ONES).all() and (pops == n).all()
            got, _, _ = check_min_edge(dens, d2, ct, r2, G.labels("own", n), rank, (f"own n={n} D={D}", r2, kind))
            assert (got != ALL_ONES).all() and ((got >> np.uint64(32)) < n).all()


@pytest.mark.parametrize("D", [1, 3, 33, 64])
def test_min_edge_round_on_lattice_clusters_and_their_transforms(dens, probe, D):
    """the round where the pruning engages (2500 rows in clusters), at the tie radii, on the plain, scaled and shifted
    lattice, random components of a few frames"""
    n = 2500
    base = G.clustered_lattice(n, D, seed=70 + D)
    d2_base = probe.pairwise_d2(base)
    comp = G.labels("any", n, seed=D)
    for k, (name, scale, shift) in enumerate(G.TRANSFORMS):
        rank = G.rank_of(G.RANKS[k % 4], n, D)
        for r2_base in G.tie_radii(d2_base, G.level_of(d2_base, 1)) + (NAN,):
            c, r2 = G.transformed(base, r2_base, scale, shift)
            d2 = probe.pairwise_d2(c)
            check_min_edge(dens, d2, gpu(c), r2, comp, rank, (f"clusters {name} D={D}", "r2", r2))


@pytest.mark.parametrize("D", [3, 10, 33, 64])
def test_a_bridge_below_r2_links_two_clusters_and_a_decoy_at_r2_does_not(dens, probe, D):
    """point 4 for the round: two clusters, one component each, joined by exactly one pair below r2 and one pair AT r2.
    Both components must report the bridge, whatever the ranks say -- also when the decoy would be lighter."""
    c, r2, side, (p, q), (d, _) = G.bridge(D)
    n = len(c)
    d2 = probe.pairwise_d2(c)
    cross = side[:, None] != side[None, :]
    assert (d2[cross] < F32(r2)).sum() == 2 and (d2[cross] == F32(r2)).sum() == 2    # (one pair each, seen from both ends)
    assert d2[p, q] < F32(r2) and d2[d, q] == F32(r2)
    ct = gpu(c)
    ids = [int(np.flatnonzero(side == s)[-1]) for s in (0, 1)]     # (named by their largest member)
    comp = np.where(side == 0, ids[0], ids[1]).astype(np.uint32)
    light = np.arange(n, dtype=np.uint32)       # the decoy lightest, the bridge heaviest
    others = [f for f in range(n) if f not in (p, q, d)]
    light[[d, q] + others + [p]] = np.arange(n, dtype=np.uint32)
    for kind, rank in [(k, G.rank_of(k, n, D)) for k in G.RANKS] + [("decoy lightest", light)]:
        got, _, _ = check_min_edge(dens, d2, ct, r2, comp, rank, (f"bridge D={D}", kind))
        key = (np.uint64(max(rank[p], rank[q])) << np.uint64(32)) | np.uint64(min(rank[p], rank[q]))
        assert got[ids[0]] == key and got[ids[1]] == key and (got != ALL_ONES).sum() == 2
        # one float further out the decoy is a pair too
        up = float(np.nextafter(F32(r2), F32(INF)))
        got, _, pairs = check_min_edge(dens, d2, ct, up, comp, rank, (f"bridge D={D}", kind, "r2 one float up"))
        assert len(pairs) == len(G.pairs_of(d2, r2)) + 1


@pytest.mark.parametrize("D", [1, 10, 64])
def test_min_edge_segments_merge_to_the_whole_round(dens, probe, D):
    """segments of 2, 3 and 8 merge by unsigned minimum / summation to the whole round -- also with more segments than
    query groups (33 rows, 8 segments)"""
    for n in (33, 257, 2000):
        c = G.clustered_lattice(n, D, seed=80 + D) if n > 257 else G.lattice(n, D, seed=80 + D + n)
        d2 = probe.pairwise_d2(c)
        ct = gpu(c)
        tie = G.tie_radii(d2, G.level_of(d2, 1))
        for r2 in (tie[1], tie[2], NAN) + ((INF,) if n <= 257 else ()):
            for lab in ("own", "any", "one"):
                comp = G.labels(lab, n, seed=D)
                rank = G.rank_of("random", n, D)
                what = (f"segments n={n} D={D}", "r2", r2, lab)
                whole, pops, _ = check_min_edge(dens, d2, ct, r2, comp, rank, what)
                for n_seg in (2, 3, 8):
                    check_segments(dens, ct, r2, comp, rank, n_seg, whole, pops, what)


def test_min_edge_round_refuses_one_row_beyond_its_limit(dens):
    """n_rows = kMinEdgeMaxRows + 1 is DC_ERR_INVALID_ARGUMENT (the queue holds 24-bit positions of the padded order) --
    called with buffers really sized for that n at one column, so that a wrongly accepted call would stay in bounds"""
    import torch
    from clustering_amd import capi
    n = MIN_EDGE_MAX_ROWS + 1
    dev = torch.device("cuda")
    coords = torch.zeros((n, 1), dtype=torch.float32, device=dev)
    comp = torch.zeros(n, dtype=torch.int32, device=dev)
    rank = torch.arange(n, dtype=torch.int32, device=dev)
    best = torch.zeros(n, dtype=torch.int64, device=dev)
    pops = torch.zeros(n, dtype=torch.int32, device=dev)
    need = int(capi.lib.dc_hip_workspace_bytes(n, 1, 1))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    args = (dens._dev(coords), n, 1, 1.0, dens._dev(comp), dens._dev(rank))
    tail = (dens._dev(best), dens._dev(pops), dens._dev(ws), need, dens._stream_ptr())
    assert capi.lib.dc_hip_radius_min_edge_dev(*args, *tail) == DC_ERR_INVALID_ARGUMENT
    assert b"n_rows <=" in capi.lib.dc_hip_last_error()
    assert capi.lib.dc_hip_radius_min_edge_segment_dev(*args, 1, 3, *tail) == DC_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert int(best.abs().max().item()) == 0 and int(pops.max().item()) == 0     # (nothing was launched)


# ---- the forest ---------------------------------------------------------------------------------------------------------
def check_forests(dens, probe, c, r2, rank, what, others=False, d2=None):
    """dc_hip_radius_forest against the contract at every threshold; others: the session's forest and the sharded
    loop's (single rank) must be the same pair set"""
    import torch
    n = len(c)
    d2 = probe.pairwise_d2(c) if d2 is None else d2
    graph = G.pairs_of(d2, r2)
    edges, rounds = dens.radius_forest(c, r2, rank)
    try:
        n_comp = G.check_forest(n, graph, rank, edges, rounds)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None
    if others:
        with dens.Session(c, n_devices=1) as s:
            e_s, rounds_s = s.radius_forest(r2, rank)
        assert np.array_equal(np.sort(G.keys(e_s, n)), np.sort(G.keys(edges, n))), (what, "session forest")
        assert rounds_s == rounds
        from clustering_amd.distributed import ShardedForest
        ct = gpu(c)
        e_d, _ = ShardedForest().run(ct, r2, torch.from_numpy(rank.astype(np.int32)).cuda())
        answered(dens, ct, what)
        assert np.array_equal(np.sort(G.keys(e_d, n)), np.sort(G.keys(edges, n))), (what, "sharded forest")
    return edges, rounds, n_comp


@pytest.mark.parametrize("kind", G.RANKS)
def test_forest_of_a_chain(dens, probe, kind):
    """point 5: 4097 frames on a line, r2 one float above 1 -- a path, whose Boruvka rounds look like nothing in the blob
    tests (identity rank: one round joins everything; random: ~log n rounds); session and sharded loop the same"""
    n = 4097
    c = G.chain(n)
    r2 = float(np.nextafter(F32(1.0), F32(INF)))
    edges, rounds, n_comp = check_forests(dens, probe, c, r2, G.rank_of(kind, n), f"chain, {kind} rank", others=True)
    assert n_comp == 1 and np.array_equal(np.sort(G.keys(edges, n)), G.keys(np.stack([np.arange(n - 1), np.arange(1, n)], 1), n))
    # exactly at 1 the chain falls apart
    edges, rounds, n_comp = check_forests(dens, probe, c, 1.0, G.rank_of(kind, n), f"chain at r2 = 1, {kind} rank")
    assert len(edges) == 0 and rounds == 1


@pytest.mark.parametrize("D", [3, 10, 33, 64])
def test_forest_of_two_cliques_a_bridge_and_a_decoy(dens, probe, D):
    """points 4 and 5: the bridge below r2 is the forest's only pair between the cliques; the decoy AT r2 is none, even
    where it is the lightest pair of all"""
    c, r2, side, (p, q), (d, _) = G.bridge(D)
    n = len(c)
    light = np.empty(n, dtype=np.uint32)
    light[[d, q] + [f for f in range(n) if f not in (p, q, d)] + [p]] = np.arange(n, dtype=np.uint32)
    for kind, rank in [(k, G.rank_of(k, n, D)) for k in G.RANKS] + [("decoy lightest", light)]:
        edges, _, n_comp = check_forests(dens, probe, c, r2, rank, f"bridge D={D}, {kind}", others=True)
        between = edges[side[edges[:, 0]] != side[edges[:, 1]]]
        assert n_comp == 1 and len(between) == 1 and set(between[0].tolist()) == {p, q}
    # with isolated frames mixed in
    ci = G.with_isolated(c)
    _, _, n_comp = check_forests(dens, probe, ci, r2, G.rank_of("random", len(ci)), f"bridge with isolated frames D={D}")
    assert n_comp == 1 + 7


@pytest.mark.parametrize("D", [2, 10, 33, 64])
def test_forest_of_a_star(dens, probe, D):
    """a hub within r2 of 2 D leaves that are mutually AT r2 or beyond: every forest pair holds the hub"""
    c, r2, hub = G.star(D)
    n = len(c)
    for kind in G.RANKS:
        edges, rounds, n_comp = check_forests(dens, probe, c, r2, G.rank_of(kind, n, D), f"star D={D}, {kind}")
        assert n_comp == 1 and (edges == hub).any(axis=1).all() and rounds == 2
    ci = G.with_isolated(c)
    _, _, n_comp = check_forests(dens, probe, ci, r2, G.rank_of("bit-reversed", len(ci)), f"star with isolated frames D={D}")
    assert n_comp == 1 + 7


@pytest.mark.parametrize("D", [1, 10, 64])
def test_forest_of_complete_and_empty_graphs(dens, probe, D):
    """2000 duplicates (complete at any r2 > 0), a lattice at r2 = inf (complete as well), and r2 of 0, NaN, -1 (no
    pair: no forest pair, one round)"""
    n = 2000
    dup = np.full((n, D), 1.0, dtype=np.float32)
    d2 = np.zeros((n, n), dtype=np.float32)
    assert (probe.pairwise_d2(dup[:64]) == 0).all()
    edges, _, n_comp = check_forests(dens, probe, dup, 1e-45, G.rank_of("random", n, D), f"duplicates D={D}", d2=d2)
    assert n_comp == 1 and len(edges) == n - 1
    c = G.clustered_lattice(601, D, seed=90 + D)
    for kind in ("reversed", "random"):
        edges, _, n_comp = check_forests(dens, probe, c, INF, G.rank_of(kind, 601, D), f"r2 = inf D={D}, {kind}")
        assert n_comp == 1
    for r2 in (0.0, NAN, -1.0):
        for data, name in ((c, "lattice"), (dup[:257], "duplicates")):
            edges, rounds, n_comp = check_forests(dens, probe, data, r2, G.rank_of("random", len(data)),
                                                  f"{name} D={D} r2={r2}")
            assert len(edges) == 0 and rounds == 1 and n_comp == len(data)


@pytest.mark.parametrize("D", [1, 33])
def test_forest_of_zero_one_and_two_rows(dens, probe, D):
    for n in (0, 1):
        edges, rounds = dens.radius_forest(np.zeros((n, D), dtype=np.float32), 1.0, np.arange(n, dtype=np.uint32))
        assert len(edges) == 0 and rounds == 0
    two = np.zeros((2, D), dtype=np.float32)
    two[1, 0] = 3.0
    for rank in (np.array([0, 1], dtype=np.uint32), np.array([1, 0], dtype=np.uint32)):
        for r2, linked in ((9.0, False), (float(np.nextafter(F32(9.0), F32(INF))), True), (INF, True), (NAN, False)):
            edges, rounds, _ = check_forests(dens, probe, two, r2, rank, f"two rows D={D} r2={r2}", others=linked)
            assert len(edges) == int(linked) and rounds == (2 if linked else 1)


# ---- the other summation orders -----------------------------------------------------------------------------------------
CHILD = r"""
import os
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from clustering_amd import capi, density as dens
from oracle.oracle import Probe
import graphref as G
import test_gpu_graph_edges as T
ORDER = sys.argv[2]
assert capi.lib.dc_hip_canon_order().decode() == ORDER, capi.lib.dc_hip_canon_order()
probe = Probe(ORDER)
for D in (3, 33, 64):
    # a tie case: pair list and one round at the float below, at and above a lattice d2
    n = 1500
    c = G.clustered_lattice(n, D, seed=11 + D)
    d2 = probe.pairwise_d2(c)
    assert (d2.view(np.uint32) == Probe("sse2").pairwise_d2(c).view(np.uint32)).all()   # (exact in both orders)
    ct = T.gpu(c)
    for r2 in G.tie_radii(d2, G.level_of(d2, 1)) + (G.NAN,):
        T.check_pairs(dens, d2, ct, r2, (ORDER, "ties", D, r2))
        T.check_min_edge(dens, d2, ct, r2, G.labels("any", n, D), G.rank_of("bit-reversed", n), (ORDER, "round", D, r2))
    # a forest case: the bridge and its decoy, and the chain
    b, r2, side, (p, q), _ = G.bridge(D)
    edges, _, n_comp = T.check_forests(dens, probe, b, r2, G.rank_of("random", len(b), D), (ORDER, "bridge", D), others=True)
    between = edges[side[edges[:, 0]] != side[edges[:, 1]]]
    assert n_comp == 1 and len(between) == 1 and set(between[0].tolist()) == {p, q}
T.check_forests(dens, probe, G.chain(4097), float(np.nextafter(np.float32(1.0), np.float32(2.0))),
                G.rank_of("random", 4097), (ORDER, "chain"), others=True)
print("ok")
"""


@pytest.mark.parametrize("order", ["avx", "fma"])
def test_graph_edges_in_the_other_orders(order):
    """a tie case and a forest case against the avx / fma libraries with the probe of that order (one process binds one
    library: a fresh child)"""
    if not os.path.exists(os.path.join(ROOT, "clustering_amd", "lib_" + order, "libdcdensity.so")):
        pytest.fail(f"clustering_amd/lib_{order}/libdcdensity.so is missing: __graft_entry__.build() makes it")
    env = dict(os.environ, DC_CANON_ORDER=order)
    env.pop("DC_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, order], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
