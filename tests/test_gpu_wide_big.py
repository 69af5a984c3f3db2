"""GPU: the wide matrix-core sweeps (65..256 columns, self and cross form) at the sizes they were written for, bit for
bit against the CPU oracle (self) and the probe's canonical d2 (cross): 4 to 64 reference shares and the seams between
the share counts, a second launch group at 1, 8 and 64 shares, row ranges that start in a later query block, ties whose
tied references lie in different shares, waves and halves of a wave, queues that fill and are drained inside push, and
statistics without extent.  Every finite call first asserts that the matrix-core kernel answered with exactly the tile
pairs of its launch -- which also proves that every share ran all its blocks.  Cases: tests/widebigref.py (their
conditions, and the unit map itself, are checked on the CPU by tests/test_wide_big_cases.py)."""
import functools

import numpy as np
import pytest

import crossref
import crosswideref as cw
import wideref
import widebigref as wb
from crossref import bits, expect_nn, expect_pops, gpu, host

pytestmark = pytest.mark.gpu
FLT_MAX = np.finfo(np.float32).max
D = 65   # the cheapest chain: 13 MFMAs


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
def the_oracle():
    from clustering_amd import capi
    from oracle.oracle import Oracle
    return Oracle(order=capi.CANON_ORDER)


def launches(radii):
    return -(-len(radii) // 8)


# ---- the self form against the oracle, over a row range ---------------------------------------------------------------------
def self_pops(dens, c, radii, lo, hi, want, what):
    """-> (tiles, mfmas, exact); want: the oracle's populations of the same range"""
    ct = gpu(c)
    got = host(dens.calculate_populations_wide(ct, radii, lo, hi)).astype(np.uint32).astype(np.uint64)
    info = dens.wide_sweep_info(ct.device)
    tiles = launches(radii) * cw.tile_pairs(len(c), len(c), lo, hi)
    assert info[:2] == (tiles, cw.nm_for(c.shape[1]) * tiles), (what, "the matrix-core kernel did not answer every block", info, tiles)
    if not (got == want).all():
        k, i = np.argwhere(got != want)[0]
        pytest.fail(f"{what}: {int((got != want).sum())} populations differ, e.g. radius {k} row {i}: {got[k, i]} != {want[k, i]}")
    return info


def self_nn(dens, c, fe, lo, hi, want, what):
    ct = gpu(c)
    got = [host(t) for t in dens.nearest_neighbors_wide(ct, gpu(fe), lo, hi)]
    info = dens.wide_sweep_info(ct.device)
    tiles = cw.tile_pairs(len(c), len(c), lo, hi)
    assert info[:2] == (tiles, cw.nm_for(c.shape[1]) * tiles), (what, "the matrix-core kernel did not answer every block", info, tiles)
    for k in (0, 2):
        g = got[k].astype(np.uint32).astype(np.uint64)
        assert (g == want[k]).all(), (what, "idx", k, np.flatnonzero(g != want[k])[:5])
        assert (bits(got[k + 1]) == bits(want[k + 1])).all(), (what, "d2", k, np.flatnonzero(bits(got[k + 1]) != bits(want[k + 1]))[:5])
    return info


@functools.lru_cache(maxsize=None)
def self_case(n_rows, lo, hi, k=3):
    """(coords, radii, free energies, the oracle's populations and neighbours of the rows [lo, hi)): once per shape"""
    o = the_oracle()
    c = wideref.blobs(n_rows, D)
    radii = cw.radii_for(D, k)
    fe = wb.fe_random(n_rows)
    return c, radii, fe, o.populations(c, radii, lo, hi), o.nearest_neighbors(c, fe, lo, hi)


# ---- the cross form against the probe ---------------------------------------------------------------------------------------
def cross_expect(Q, R, radii, fe_q, fe_r, piece=4096):
    """populations and neighbours of every query from the probe's d2, a piece of Q at a time (a 65 700 x 1 920 block of
    d2 and the masks over it are not held at once)"""
    pops, nn = [], []
    for a in range(0, len(Q), piece):
        d2 = wb.rect_d2(the_probe(), Q[a:a + piece], R)
        pops.append(expect_pops(d2, radii))
        nn.append(expect_nn(d2, fe_q[a:a + piece], fe_r))
    return np.hstack(pops), [np.concatenate([p[k] for p in nn]) for k in range(4)]


def in_range(want, lo, hi, n_r):
    """the expectation of a call over the query rows [lo, hi): zeros / none outside"""
    pops, nn = want
    rows = np.zeros(pops.shape[1], dtype=bool)
    rows[lo:hi] = True
    return np.where(rows, pops, 0), [np.where(rows, nn[k], n_r + 1 if k % 2 == 0 else F32_MAX) for k in range(4)]


F32_MAX = np.float32(FLT_MAX)


def cross_check(dens, Q, R, radii, fe_q, fe_r, want, lo=0, hi=None, what=""):
    """both sweeps of the cross form over the query rows [lo, hi) -> (info of the populations, info of the neighbours)"""
    hi = len(Q) if hi is None else hi
    pops, nn = in_range(want, lo, hi, len(R))
    q, r = gpu(Q), gpu(R)
    tiles = cw.tile_pairs(len(Q), len(R), lo, hi)
    nm = cw.nm_for(Q.shape[1])
    got = host(dens.calculate_populations_against_wide(q, r, radii, lo, hi))
    info_p = dens.wide_against_info(q.device)
    assert info_p[:2] == (launches(radii) * tiles, nm * launches(radii) * tiles), (what, "populations: not every block was swept", info_p, tiles)
    if not (got == pops).all():
        k, i = np.argwhere(got != pops)[0]
        pytest.fail(f"{what}: {int((got != pops).sum())} populations differ, e.g. radius {k} query {i}: {got[k, i]} != {pops[k, i]}")
    got = dens.nearest_reference_wide(q, r, gpu(fe_q), gpu(fe_r), lo, hi)
    info_n = dens.wide_against_info(q.device)
    assert info_n[:2] == (tiles, nm * tiles), (what, "neighbours: not every block was swept", info_n, tiles)
    crossref.same_nn(got, nn, what)
    return info_p, info_n


@functools.lru_cache(maxsize=None)
def seam_sets(n_cols):
    """130 queries and 65 537 references of one draw; the seam cases take prefixes of the reference"""
    n_r = 65537 if n_cols == D else 8192
    Q, R = cw.blob_sets(n_cols, 130, n_r)
    fe_q, fe_r = cw.fe_pair(130, n_r)
    return Q, R, fe_q, fe_r, wb.rect_d2(the_probe(), Q, R)


SEAMS = [(3968, D), (3969, D), (4100, D), (8192, D), (8192, 100), (16384, D), (32768, D), (65408, D), (65409, D), (65536, D), (65537, D)]


@pytest.mark.parametrize("n_r,n_cols", SEAMS)
def test_share_counts_on_both_sides_of_every_seam(dens, n_r, n_cols):
    """31 | 32, 33, 64, 128, 256, 511 | 512 | 513 reference blocks: 2 | 4, 4, 8, 16, 32, 32 | 64 | 64 shares -- at 31, 33,
    511 and 513 blocks the shares hold different numbers of blocks -- the last block of the odd sizes holding one row; at
    100 columns 19 MFMAs: an odd number of LDS chunks, the last with three"""
    Q, R, fe_q, fe_r, d2 = seam_sets(n_cols)
    R, fe_r, d2 = np.ascontiguousarray(R[:n_r]), np.ascontiguousarray(fe_r[:n_r]), d2[:, :n_r]
    radii = cw.radii_for(n_cols, 3)
    want = expect_pops(d2, radii), expect_nn(d2, fe_q, fe_r)
    assert wb.shares_of_rows(n_r) == {31: 2, 32: 4, 33: 4, 64: 8, 128: 16, 256: 32, 511: 32, 512: 64, 513: 64}[wb.blocks(n_r)]
    cross_check(dens, Q, R, radii, fe_q, fe_r, want, what=("seam", n_r, n_cols))


def test_a_second_launch_group_with_eight_shares(dens):
    """8 320 rows: 65 reference blocks in 8 shares -- share 0 holds 9 blocks, the others 8 -- and 65 query blocks: the
    65th opens the second group of 512 workgroups"""
    n = 8320
    assert wb.shares_of_rows(n) == 8 and wb.units(8, 65)[0] == 2 * wb.GROUP
    c, radii, fe, pops, nn = self_case(n, 0, n)
    self_pops(dens, c, radii, 0, n, pops, "8 shares, 2 groups")
    self_nn(dens, c, fe, 0, n, nn, "8 shares, 2 groups")


BIG = 65664   # 513 blocks: 64 shares, share 0 holds 9 blocks, the others 8


def test_a_second_launch_group_with_64_shares(dens):
    """the rows [64 500, 65 664) of 65 664: 10 query blocks against 513 reference blocks in 64 shares, 8 query blocks to
    a group"""
    lo, hi = 64500, BIG
    assert wb.shares_of_rows(BIG) == 64 and wb.units(64, 10)[0] == 2 * wb.GROUP and hi // 128 - lo // 128 == 10
    c, radii, fe, pops, nn = self_case(BIG, lo, hi)
    self_pops(dens, c, radii, lo, hi, pops, "64 shares, 2 groups")
    self_nn(dens, c, fe, lo, hi, nn, "64 shares, 2 groups")


@pytest.mark.parametrize("lo,hi,q_blocks", [(33000, 33100, 2), (33030, 33100, 1)])
def test_a_range_in_the_middle_with_64_shares(dens, lo, hi, q_blocks):
    """a range that starts inside query block 257 -- [33 000, 33 100) runs on over the block boundary at 33 024, the
    other one ends inside block 258 -- and the counters of exactly the blocks it touches, each against all 513"""
    assert (hi + 127) // 128 - lo // 128 == q_blocks
    c, radii, fe, pops, nn = self_case(BIG, lo, hi)
    info_p = self_pops(dens, c, radii, lo, hi, pops, "mid-block range")
    info_n = self_nn(dens, c, fe, lo, hi, nn, "mid-block range")
    assert info_p[0] == 16 * q_blocks * 513 and info_n[0] == 16 * q_blocks * 513


@functools.lru_cache(maxsize=None)
def long_query_case(n_q, n_r, k=3):
    Q, R = cw.blob_sets(D, n_q, n_r)
    fe_q, fe_r = cw.fe_pair(n_q, n_r)
    radii = cw.radii_for(D, k) + [1e30]
    return Q, R, radii, fe_q, fe_r, cross_expect(Q, R, radii, fe_q, fe_r)


@pytest.mark.parametrize("n_r", [40, 1920])
def test_a_second_launch_group_with_one_share(dens, n_r):
    """65 700 queries: 514 query blocks, one share -- 512 query blocks to a group.  (1 920 references: 15 blocks, the
    most one share holds)"""
    n_q = 65700
    assert wb.shares_of_rows(n_r) == 1 and wb.units(1, wb.blocks(n_q))[0] == 2 * wb.GROUP
    Q, R, radii, fe_q, fe_r, want = long_query_case(n_q, n_r)
    assert (want[0][3] == n_r).all(), "every reference lies inside a radius beyond every float"
    cross_check(dens, Q, R, radii, fe_q, fe_r, want, what=("one share, 2 groups", n_r))


def test_many_query_blocks_by_64_shares(dens):
    """1 100 queries against 65 537 references: 9 query blocks x 64 shares, the ninth in a group of its own"""
    n_q, n_r = 1100, 65537
    assert wb.shares_of_rows(n_r) == 64 and wb.units(64, wb.blocks(n_q))[0] == 2 * wb.GROUP
    Q, R, radii, fe_q, fe_r, want = long_query_case(n_q, n_r)
    cross_check(dens, Q, R, radii, fe_q, fe_r, want, what="9 query blocks x 64 shares")


@pytest.mark.parametrize("lo,hi", [(1030, 1100), (1023, 1025)])
def test_a_query_range_that_starts_in_a_later_block(dens, lo, hi):
    n_q, n_r = 1100, 65537
    Q, R, radii, fe_q, fe_r, want = long_query_case(n_q, n_r)
    info_p, info_n = cross_check(dens, Q, R, radii, fe_q, fe_r, want, lo, hi, what=("range", lo, hi))
    assert info_n[0] == 16 * (2 if lo == 1023 else 1) * 513


# ---- ties across shares ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_r,n_shares", [(8192, 8), (65664, 64)])
def test_ties_between_references_of_different_shares_cross(dens, n_r, n_shares):
    case = wb.star_across_shares(n_r, D, n_shares)
    R, fe_r = case["R"], case["fe_r"]
    Q, fe_q, rows = wb.star_queries(case, 130, D)
    radii = cw.radii_for(D, 2) + [2.0 ** -6, float(np.nextafter(np.float32(2.0 ** -6), np.float32(1)))]
    want = cross_expect(Q, R, radii, fe_q, fe_r)
    assert wb.shares_of_rows(n_r) == n_shares
    cross_check(dens, Q, R, radii, fe_q, fe_r, want, what=("ties", n_r))
    pops, nn = want
    (_, ring0, _), (_, ring1, _) = case["stars"]
    _, lo, hi, _ = case["dup"]
    assert (nn[0][rows[0]], nn[2][rows[0]]) == (ring0[0], ring0[0]) and nn[1][rows[0]] == wb.TIE_D2
    assert (nn[0][rows[1]], nn[2][rows[1]]) == (ring1[0], ring1[4]) and nn[1][rows[1]] == wb.TIE_D2 and nn[3][rows[1]] == wb.TIE_D2
    assert (nn[0][rows[2]], nn[2][rows[2]]) == (lo, lo) and nn[1][rows[2]] == 0
    # on the radius 2^-6 itself no ring row counts, one ulp above it all six do
    assert pops[2][rows[0]] == 0 and pops[3][rows[0]] == 6 and pops[2][rows[2]] == 2


@pytest.mark.parametrize("n_r,n_shares", [(8192, 8), (65664, 64)])
def test_ties_between_references_of_different_shares_self(dens, n_r, n_shares):
    case = wb.star_across_shares(n_r, D, n_shares, self_form=True)
    c, fe = case["R"], case["fe_r"]
    lo, hi = case["span"]
    o = the_oracle()
    radii = cw.radii_for(D, 2) + [2.0 ** -6, float(np.nextafter(np.float32(2.0 ** -6), np.float32(1)))]
    pops, nn = o.populations(c, radii, lo, hi), o.nearest_neighbors(c, fe, lo, hi)
    self_pops(dens, c, radii, lo, hi, pops, ("ties", n_r))
    self_nn(dens, c, fe, lo, hi, nn, ("ties", n_r))
    rows = case["centres"]
    (_, ring0, _), (_, ring1, _) = case["stars"]
    _, dlo, dhi, _ = case["dup"]
    assert (nn[0][rows[0]], nn[2][rows[0]]) == (ring0[0], ring0[0]) and nn[1][rows[0]] == wb.TIE_D2
    assert (nn[0][rows[1]], nn[2][rows[1]]) == (ring1[0], ring1[4]) and nn[3][rows[1]] == wb.TIE_D2
    assert (nn[0][rows[2]], nn[2][rows[2]]) == (dlo, dlo) and nn[1][rows[2]] == 0
    assert pops[2][rows[0]] == 1 and pops[3][rows[0]] == 7


# ---- queues that fill ---------------------------------------------------------------------------------------------------
def full_queue(info, units, what):
    """A wave that never drains inside push hands at most kWideQueue pairs to the exact path (its final drain), a
    workgroup of four waves 4 x 256: more exact pairs than that per (query block, share) unit swept, and the drain
    inside push has run."""
    tiles, mfmas, exact = info
    print(f"{what}: {exact} exact pairs = {100.0 * exact / (1024 * tiles):.2f} % of the {1024 * tiles} evaluated, "
          f"{exact / (wb.QUEUE * 4 * units):.1f} x what {units} workgroups hold without a drain inside push")
    assert exact > wb.QUEUE * 4 * units, (what, exact, units)


@pytest.mark.parametrize("n_cols", [65, 256])
def test_a_full_queue_is_drained_inside_push_self(dens, n_cols):
    case = wb.outlier_case(500, n_cols)
    c, radii = case["c"], case["radii"]
    n = len(c)
    o = the_oracle()
    for rad in (radii[:1], radii[:4], radii):
        info = self_pops(dens, c, rad, 0, n, o.populations(c, rad), ("full queue", n_cols, len(rad)))
        full_queue(info, wb.swept_units(n, 0, n), f"D={n_cols} self, {len(rad)} radii")
    info = self_pops(dens, c, radii, 100, 400, o.populations(c, radii, 100, 400), ("full queue, range", n_cols))
    full_queue(info, wb.swept_units(n, 100, 400), f"D={n_cols} self, rows [100, 400)")
    fe = wb.fe_random(n)
    info = self_nn(dens, c, fe, 0, n, o.nearest_neighbors(c, fe), ("full queue, neighbours", n_cols))
    full_queue(info, wb.swept_units(n, 0, n), f"D={n_cols} self, neighbours")
    info = self_nn(dens, c, fe, 100, 400, o.nearest_neighbors(c, fe, 100, 400), ("full queue, neighbours, range", n_cols))
    full_queue(info, wb.swept_units(n, 100, 400), f"D={n_cols} self, neighbours of [100, 400)")


@pytest.mark.parametrize("n_cols", [65, 256])
def test_a_full_queue_is_drained_inside_push_cross(dens, n_cols):
    case = wb.outlier_case(500, n_cols)
    Q, R, radii = case["Q"], case["R"], case["radii"]
    fe_q, fe_r = cw.fe_pair(len(Q), len(R))
    units = wb.swept_units(len(R), 0, len(Q))
    for rad in (radii[:1], radii[:4], radii):
        want = cross_expect(Q, R, rad, fe_q, fe_r)
        info_p, info_n = cross_check(dens, Q, R, rad, fe_q, fe_r, want, what=("full queue", n_cols, len(rad)))
        full_queue(info_p, units, f"D={n_cols} cross, {len(rad)} radii")
    full_queue(info_n, units, f"D={n_cols} cross, neighbours")


# ---- statistics without extent ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_ulp", [False, True])
def test_identical_rows_self(dens, one_ulp):
    """M = 0 (or a few ulp^2): the data is not flagged, the scale exponent is far up, a finite radius scales beyond FLT_MAX"""
    c = wb.identical_rows(300, 100, one_ulp)
    o = the_oracle()
    radii = wb.DEGENERATE_RADII
    self_pops(dens, c, radii, 0, len(c), o.populations(c, radii), ("identical rows", one_ulp))
    self_pops(dens, c, radii[4:5], 37, 171, o.populations(c, radii[4:5], 37, 171), ("identical rows, 1e15 alone", one_ulp))
    for fe in (wb.fe_random(len(c)), wideref.fe_all_equal(len(c))):
        self_nn(dens, c, fe, 0, len(c), o.nearest_neighbors(c, fe), ("identical rows", one_ulp))


@pytest.mark.parametrize("one_ulp", [False, True])
def test_identical_rows_cross(dens, one_ulp):
    c = wb.identical_rows(300, 100, one_ulp)
    Q, R = np.ascontiguousarray(c[120:]), np.ascontiguousarray(c[:120])   # (the odd row of the variant is a query)
    fe_q, fe_r = cw.fe_pair(len(Q), len(R))
    radii = wb.DEGENERATE_RADII
    want = cross_expect(Q, R, radii, fe_q, fe_r)
    cross_check(dens, Q, R, radii, fe_q, fe_r, want, what=("identical rows", one_ulp))
    Q, R = R, Q
    want = cross_expect(Q, R, radii, fe_r, fe_q)
    cross_check(dens, Q, R, radii, fe_r, fe_q, want, what=("identical rows, the odd row a reference", one_ulp))


def test_small_data_under_a_radius_that_scales_beyond_every_float(dens):
    """blob frames scaled by 1e-6: S ~ 2^66, and fl32(1e15^2) S = inf -- every finite accumulator is inside"""
    from test_gpu_wide_mfma import blob_reference
    c, radii, _, _, _ = blob_reference(300, 100, 3)
    f = np.float32(1e-6)
    c = np.ascontiguousarray((c * f).astype(np.float32))
    radii = [float(np.float32(r) * f) for r in radii] + [1e15, 1e-30]
    o = the_oracle()
    pops = o.populations(c, radii)
    assert (pops[3] == len(c)).all() and (pops[4] == 1).all() and 1 < int(pops[0].max()) < len(c)
    self_pops(dens, c, radii, 0, len(c), pops, "scaled 1e-6, radius 1e15")
    fe = wb.fe_random(len(c))
    Q, R = np.ascontiguousarray(c[:130]), np.ascontiguousarray(c[130:])
    want = cross_expect(Q, R, radii, fe[:130], fe[130:])
    assert (want[0][3] == len(R)).all()
    cross_check(dens, Q, R, radii, fe[:130], fe[130:], want, what="scaled 1e-6, radius 1e15")


# ---- a small call behind a big one in the same cached workspace ---------------------------------------------------------------
def test_a_small_call_behind_the_stale_images_of_a_big_one_self(dens):
    import test_gpu_wide_mfma as small
    lo, hi = 33000, 33100
    c, radii, fe, pops, nn = self_case(BIG, lo, hi)
    self_pops(dens, c, radii, lo, hi, pops, "the big call")
    sc, sradii, spops, sfe, snn = small.blob_reference(300, 100, 3)
    self_pops(dens, sc, sradii, 0, 300, spops, "the small call behind it")
    self_nn(dens, c, fe, lo, hi, nn, "the big call, neighbours")
    self_nn(dens, sc, sfe, 0, 300, snn, "the small call behind it, neighbours")
    self_pops(dens, sc, sradii, 37, 171, the_oracle().populations(sc, sradii, 37, 171), "the small call again, a range")


def test_a_small_call_behind_the_stale_images_of_a_big_one_cross(dens):
    Q, R, radii, fe_q, fe_r, want = long_query_case(1100, 65537)
    cross_check(dens, Q, R, radii, fe_q, fe_r, want, 1023, 1025, what="the big call")
    sQ, sR = cw.blob_sets(100, 33, 127)
    sfq, sfr = cw.fe_pair(33, 127)
    sradii = cw.radii_for(100, 3)
    swant = cross_expect(sQ, sR, sradii, sfq, sfr)
    cross_check(dens, sQ, sR, sradii, sfq, sfr, swant, what="the small call behind it")
    cross_check(dens, Q, R, radii, fe_q, fe_r, want, 1030, 1100, what="the big call again")
    cross_check(dens, sQ, sR, sradii, sfq, sfr, swant, 5, 30, what="the small call again, a range")
