"""CPU: the premises of the built cases of tests/test_gpu_cross_pruned_big.py (tests/crossbigref.py), from the probe's
canonical d2 and the restated orders and share counts alone: tile counts per share, the scan round of every expected
partner, exact lattice distances, the order positions at 2^24, and that no expectation is degenerate."""
import numpy as np
import pytest

import crossbigref as cb
import crossprunedref as cp
from crossref import F32, FLT_MAX, block_d2, expect_nn, expect_pops, sets, square


@pytest.fixture(scope="module")
def probe():
    from clustering_amd import capi
    from oracle.oracle import Probe
    return Probe(capi.CANON_ORDER)


def test_first_position_is_the_order(probe):
    Q, R = sets(3, 100, 3000, seed=5)
    fe_r = np.random.default_rng(1).uniform(0, 1, len(R)).astype(np.float32)
    for fe in (None, fe_r):
        _, _, pos = cb.ref_order(Q, R, cb.NN_CELL, fe)
        _, key = cb.ref_keys(Q, R, cb.NN_CELL, fe)
        for rows in ([7], [2999, 5, 77], np.arange(100, 900)):
            assert cb.first_position(key, rows) == pos[np.asarray(rows)].min()


def test_classes_and_pieces(probe):
    """one width per class of instance, and the referee in pieces is the referee"""
    assert [cb.nm_for(D) for D in cb.CLASS_WIDTHS] == [1, 2, 4, 5]
    assert [cb.instance_class(D) for D in cb.CLASS_WIDTHS] == ["full chains", "early, 1 coarse", "early, 2 coarse", "single buffer"]
    assert [cb.tq_of(cb.nm_for(D)) for D in cb.CLASS_WIDTHS] == [6, 6, 4, 4]
    for D in cb.CLASS_WIDTHS:
        Q, R = sets(D, 100, 700, seed=D)
        assert (cb.big_d2(probe, Q, R, chunk=97).view(np.uint32) == block_d2(probe, Q, R).view(np.uint32)).all()


# ---- A ------------------------------------------------------------------------------------------------------------------
def rounds_wanted(layout):
    return {"A1": {1}, "A2": {0}, "end": {0}, "A3": {0, 1}, "A3b": {1, 2}}[layout]


@pytest.mark.parametrize("n_r", cb.A_SIZES)
@pytest.mark.parametrize("D", cb.CLASS_WIDTHS)
def test_round_layouts(probe, D, n_r):
    T = cb.tiles(n_r)
    assert T == {16384: 512, 16385: 513, 32768: 1024, 32769: 1025}[n_r]
    # one share: the neighbour sweep by its own floor, the population sweep under DC_SHARE_FLOOR = 2000
    assert cb.nn_shares(300, n_r, D) == 1 and cb.pop_shares(300, n_r, D, 2000) == 1 and cb.pop_shares(300, n_r, D) > 1
    r_max = max(cb.A_RADII)
    for layout in cb.A_LAYOUTS[n_r]:
        c = cb.case_a(D, n_r, layout)
        Q, R, boundary, tie = c["Q"], c["R"], c["boundary"], c["tie"]
        assert 150 <= len(Q) <= 400 and Q[:, 0].min() >= 0 and Q[:, 0].max() <= R[:, 0].max()
        d2 = cb.big_d2(probe, Q, R)
        want = rounds_wanted(layout)
        # the orders without free energies: the index, but for the two rows of the tie
        for frames in (cb.POP_CELL, cb.NN_CELL):
            cell, order, pos = cb.ref_order(Q, R, frames)
            assert abs(float(cell) / (frames * float(cb.H)) - 1.0) < 1e-6
            moved = np.flatnonzero(pos != np.arange(n_r))
            assert sorted(moved) == (sorted(tie) if tie else []), (layout, frames, moved[:5])
            if tie:
                assert tie[0] < tie[1] and pos[tie[0]] == boundary and pos[tie[1]] == boundary - 1
        # populations: the rows inside the largest radius, by round
        pops = expect_pops(d2, cb.A_RADII)
        assert (pops > 0).any(axis=1).all(), layout
        rows = np.flatnonzero((d2 < square(r_max)).any(axis=0))
        _, _, pos = cb.ref_order(Q, R, cb.POP_CELL)
        assert set(cb.round_of(pos[rows])) == want, (layout, set(cb.round_of(pos[rows])))
        part_tiles = set(pos[rows] // 32)
        if layout in ("A3", "A3b"):
            assert {boundary // 32 - 1, boundary // 32} <= part_tiles
        if layout == "end":
            assert T - 1 in part_tiles
        # A1 / A2: no tile of the other round is within the largest radius (x 1.001) of any query: that round's scan
        # keeps nothing for any query group
        other = R[pos < boundary, 0] if layout == "A1" else R[pos >= boundary, 0] if layout == "A2" else None
        if layout == "A1":
            assert Q[:, 0].min() - other.max() > 1.001 * r_max
        if layout == "A2":
            assert other.min() - Q[:, 0].max() > 1.001 * r_max
        # neighbours with random free energies: nn and hd by round, in the order WITH free energies
        fe_q, fe_r = cb.rand_fe(len(Q), n_r, D)
        exp = expect_nn(d2, fe_q, fe_r)
        assert (exp[2] != n_r + 1).all(), layout
        cell, _, pos_fe = cb.ref_order(Q, R, cb.NN_CELL, fe_r)
        got = set(cb.round_of(pos_fe[exp[0]])) | set(cb.round_of(pos_fe[exp[2]]))
        assert got == want, (layout, got)
        if layout in ("A1", "A2"):
            # ... and no ring reaches the other round: the first ring ends at max(group extent, cell)^2 -- at most the
            # extent of all queries -- and every incumbent is inside it
            reach = max(float(np.ptp(Q[:, 0])), float(cell)) * 1.001
            assert max(exp[1].max(), exp[3].max()) < 0.99 * float(cell) ** 2
            if layout == "A1":
                assert Q[:, 0].min() - reach > other.max()
            else:
                assert Q[:, 0].max() + reach < other.min()
        if tie:
            # the same d2 in the last tile of one round and the first tile of the next, the lower index in the later
            lo, hi = tie
            tq = np.flatnonzero((d2[:, lo] == d2[:, hi]) & (d2[:, lo] == d2.min(axis=1)))
            assert len(tq) >= 32 and (exp[0][tq] == lo).all()
            others = np.delete(d2[tq], [lo, hi], axis=1)
            assert (others.min(axis=1) > d2[tq, lo]).all()
            fq, fr = cb.tie_fe_across(len(Q), n_r, lo, hi)
            hd = expect_nn(d2, fq, fr)
            assert (hd[2][tq] == lo).all() and (hd[2] != n_r + 1).all()
            for fe in (None, fr):
                _, _, p = cb.ref_order(Q, R, cb.NN_CELL, fe)
                assert p[lo] // 32 == boundary // 32 and p[hi] // 32 == boundary // 32 - 1, (layout, fe is None, p[lo], p[hi])


@pytest.mark.parametrize("D", cb.CLASS_WIDTHS)
def test_a4_nn_and_hd_lie_in_different_rounds(probe, D):
    for far_round in (0, 1):
        Q, R, fe_q, fe_r, special = cb.case_a4(D, far_round)
        assert cb.nn_shares(len(Q), len(R), D) == 1
        exp = expect_nn(cb.big_d2(probe, Q, R), fe_q, fe_r)
        _, _, pos = cb.ref_order(Q, R, cb.NN_CELL, fe_r)
        assert (exp[2] == special).all() and (fe_r < F32(0.5)).sum() == 1
        assert set(cb.round_of(pos[exp[0]])) == {1 - far_round} and cb.round_of(pos[special]) == far_round


# ---- B ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", cb.CLASS_WIDTHS)
def test_share_counts(D):
    seen = []
    for n_q, n_r in cb.B_SHAPES:
        for n_sel in (n_q, n_q - n_q // 5 - n_q // 7):
            n = cb.pop_shares(n_sel, n_r, D, cb.B_FLOOR)
            assert 1 < n <= cb.MAX_SHARES and cb.tiles(n_r) % n != 0 and n_r % 32 != 0
            seen.append(n)
    assert max(seen) == cb.MAX_SHARES
    g, _ = cp.lattice_radii()
    Q, R = cp.lattice_sets(D, g)
    assert cb.pop_shares(len(Q), len(R), D, cb.B_FLOOR) > 1
    # the joined case: two shares of 625 tiles, two rounds each, in both sweeps
    T = cb.tiles(cb.JOIN_ROWS)
    assert T == 1250
    for n in (cb.pop_shares(300, cb.JOIN_ROWS, D, cb.JOIN_FLOOR), cb.nn_shares(300, cb.JOIN_ROWS, D, cb.JOIN_FLOOR)):
        assert n == 2 and set(cb.round_of(32 * np.arange(T), n)) == {0, 1} and T // n > cb.LIST_CAP


# ---- C ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", cb.CLASS_WIDTHS)
def test_every_pair_on_the_radius(probe, D):
    for n_r in cb.C_SIZES:
        Q, R, g, radii = cb.case_c(D, n_r)
        assert len(Q) == 192
        d2 = block_d2(probe, Q, R)
        assert (d2 == F32(g * g) / F32(64.0)).all()
        pops = expect_pops(d2, radii)
        assert (pops[0] == 0).all() and (pops[1] == n_r).all() and (pops[2] == 0).all()   # r_at, r_above, r_below
        T = cb.tiles(n_r)
        for where, tile in (("first", 0), ("middle", (T - 1) // 2), ("last", T - 1)):
            fe_q, fe_r, k0 = cb.c_fe(n_r, where)
            exp = expect_nn(d2, fe_q, fe_r)
            assert (exp[0] == 0).all() and (exp[2] == k0).all()
            _, _, pos = cb.ref_order(Q, R, cb.NN_CELL, fe_r)
            assert abs(int(pos[k0]) // 32 - tile) <= (1 if where == "middle" else 0), (n_r, where, pos[k0])
    assert cb.pop_shares(192, 2048, D, cb.B_FLOOR) > 1 and cb.nn_shares(192, 2048, D, cb.B_FLOOR) > 1


# ---- D ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [3, 10])
def test_duplicates_across_rounds(probe, D):
    Q, R, which = cb.case_d(D)
    assert cb.tiles(len(R)) == 625 and cb.nn_shares(len(Q), len(R), D) == 1 and cb.pop_shares(len(Q), len(R), D, 2000) == 1
    _, _, pos = cb.ref_order(Q, R, cb.POP_CELL)
    assert (pos == np.arange(len(R))).all()
    for k in range(50):
        p = pos[which == k]
        assert len(p) == 400 and set(cb.round_of(p)) == {0, 1} and len(set(p // 32)) > 200
    d2 = cb.big_d2(probe, Q, R)
    exp = expect_nn(d2)
    first = np.array([np.flatnonzero(which == k)[0] for k in range(50)])
    assert (exp[0] == first[which[exp[0]]]).all() and (exp[1][:150] == 0).all() and (exp[1][150:] > 0).all()
    pops = expect_pops(d2, [0.05])
    assert (pops[0][:150] >= 400).all() and (pops[0] % 400 == 0).all()
    # with free energies the copies are spread by free energy, over both rounds all the same
    fe_q, fe_r = cb.rand_fe(len(Q), len(R), D)
    _, _, pos = cb.ref_order(Q, R, cb.NN_CELL, fe_r)
    assert all(set(cb.round_of(pos[which == k])) == {0, 1} for k in range(50))
    assert (expect_nn(d2, fe_q, fe_r)[2] != len(R) + 1).any()


# ---- E ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_r", cb.E_SIZES)
def test_the_last_reference_that_is_taken(probe, n_r):
    assert cb.tiles(n_r) * 32 == cb.MAX_POS and (n_r % 32 == 0) == (n_r == cb.MAX_POS)   # taken; 2^24 + 1 is not
    Q, R, fe_q, fe_r = cb.case_e(n_r)
    # numpy's float32 (q - r)^2 is the probe's d2 in one column, on a sample of this data that holds the partners' end
    cand = cb.e_candidates(Q, R)
    sample = np.concatenate([cand[R[cand, 0] > Q[:, 0].min() - F32(0.2)][:2048], np.arange(2048)])
    assert 2500 < len(sample) <= 4096
    d2 = block_d2(probe, Q, R[sample])
    mine = np.stack([cb.e_d2(Q, R, i)[sample] for i in range(len(Q))])
    assert (d2.view(np.uint32) == mine.view(np.uint32)).all()
    radii, (qi, rj) = cb.e_radii(Q, R)
    pops, exp, inside = cb.e_expect(Q, R, fe_q, fe_r, radii)
    assert cb.e_d2(Q, R, qi)[rj] == square(radii[1]) and pops[2, qi] == pops[1, qi] + 1 and pops[0, qi] == pops[1, qi]
    assert (pops[3] > 0).all() and (exp[2] != n_r + 1).any() and (exp[2] == n_r + 1).any() and (exp[1][:8] == 0).all()
    # the partners lie in the last tiles of both orders, at positions with the top bits set
    _, key = cb.ref_keys(Q, R, cb.POP_CELL)
    assert cb.first_position(key, np.concatenate(inside + [[rj]])) >= n_r - cb.E_TOP
    has = exp[2] != n_r + 1
    _, key = cb.ref_keys(Q, R, cb.NN_CELL, fe_r)
    assert cb.first_position(key, np.concatenate([exp[0], exp[2][has]])) >= n_r - cb.E_TOP
    _, key = cb.ref_keys(Q, R, cb.NN_CELL)
    assert cb.first_position(key, exp[0]) >= n_r - cb.E_TOP > cb.MAX_POS // 2
    assert exp[3][~has].max() == exp[3][~has].min() == FLT_MAX
