"""CPU: the premises of the resident reference's GPU cases at 257..1024 columns (tests/xreferenceref.py) -- the batches are
what they say, the tail outlier passes a gate of four columns per lane and not one of sixteen, the stretched data prunes
under the reference-only order, every case sends pairs to the exact path, and the float64 range the exact-pair counter is
held to can tell a window formed from M_ref, or one twice too wide, from the right one."""
import numpy as np
import pytest

import crosswidepruneref as cp
import crosswideref as cw
import xreferenceref as ref

ALL_COLS = ref.COLS + ref.GATE_COLS


@pytest.mark.parametrize("n_cols", ALL_COLS)
def test_the_kinds_of_batch(n_cols):
    R = ref.reference_rows(1500, n_cols)
    m = ref.m_ref(R)
    limit = ref.m_res(R)
    gate = lambda X: ref.norms2(X, R).astype(np.float32).astype(np.float64) * ref.GATE_MARGIN   # what the gate compares with M_res
    Q = ref.ordinary_batch(R, 300)
    assert (gate(Q) < 0.86 * m).all() and len({r.tobytes() for r in Q} & {r.tobytes() for r in R}) == 0
    H = ref.headroom_batch(R, 300)
    moved = np.flatnonzero((H != Q).any(axis=1))
    assert len(moved) == 4 and ref.outside_box(H, R)[moved].all(), "outside the reference's box in columns 0 / 1"
    assert (gate(H)[moved] > 2.1 * m).all() and (gate(H) < 0.6 * limit).all(), "at 2.2 M_ref: inside M_res = 4 M_ref with room"
    B = ref.beyond_batch(R, 300)
    far = np.flatnonzero((B != Q).any(axis=1))
    assert len(far) == 1 and gate(B)[far[0]] > 1.5 * limit and np.isfinite(B).all(), "at 7 M_ref: beyond M_res by far more than the margin"
    assert (np.delete(gate(B), far) < 0.86 * m).all()


@pytest.mark.parametrize("n_cols", ALL_COLS)
def test_the_tail_outlier_is_beyond_m_res_only_in_the_columns_from_256_on(n_cols):
    R = ref.reference_rows(1500, n_cols)
    T, row = ref.tail_outlier_batch(R, 300)
    limit = ref.m_res(R)
    full, head = ref.norms2(T, R), ref.head_norms2(T, R)
    assert full[row] > 1.2 * limit, "beyond M_res as the gate of these widths sums it"
    assert head[row] * ref.GATE_MARGIN < 1e-6 * limit, "a gate still reading four slots (columns 0..255) would pass it"
    assert (np.delete(full, row) < 0.86 * ref.m_ref(R)).all() and np.isfinite(T).all()
    assert (T[row, :256] == ref.means(R)[:256]).all() and T[row, n_cols - 1] != ref.means(R)[n_cols - 1]


@pytest.mark.parametrize("n_cols", ref.COLS)
def test_the_stretched_data_prunes_under_the_reference_only_order(n_cols):
    Q, R = ref.split_sets(1500, 1500, n_cols)
    perm_q, perm_r = ref.reference_order(Q, R)
    lo, hi = cp.tile_bounds(Q, R, perm_q, perm_r, ref.radii_for(n_cols))
    g = cp.gaps(Q, R, perm_q, perm_r)
    assert 0 < lo <= hi < 16 * g.size, "strictly fewer than all tile pairs"
    assert hi <= 16 * g.size // 2


@pytest.mark.parametrize("n_cols", ALL_COLS)
def test_every_case_sends_pairs_to_the_exact_path(n_cols):
    """at least one pair inside the band in float64, on the blob data of the sequence tests"""
    R = ref.reference_rows(1500, n_cols)
    Q = ref.ordinary_batch(R, 300)
    radii = cw.radii_for(n_cols, 3)
    perm_q, perm_r = ref.reference_order(Q, R)
    (sure, may), = ref.window_counts(n_cols, Q, R, perm_q, perm_r, radii, [0.5])
    assert sure > 100 and may >= sure, "well inside the window: within half its half-width"
    assert ref.windows_apart(n_cols, R, radii)


@pytest.mark.parametrize("n_cols", ref.COLS)
def test_the_exact_pair_range_can_tell_a_wrong_window(n_cols):
    """[#{|d2 - r^2| < (1 - f) eps}, #{|d2 - r^2| < (1 + f) eps}] with eps from M_res = 4 M_ref: a window formed from M_ref
    counts below it, one twice too wide above it; the windows of the three radii do not meet, so no pair counts twice"""
    Q, R = ref.split_sets(1500, 1500, n_cols)
    radii, f = ref.radii_for(n_cols), ref.F_EXACT[n_cols]
    perm_q, perm_r = ref.reference_order(Q, R)
    assert 0.0 < f < 0.05 and ref.windows_apart(n_cols, R, radii)
    (lower, _), (inside, _), (_, upper), (_, twice) = ref.window_counts(n_cols, Q, R, perm_q, perm_r, radii, [1.0 - f, 1.0, 1.0 + f, 2.0])
    (_, from_m_ref), = ref.window_counts(n_cols, Q, R, perm_q, perm_r, radii, [1.0], m=ref.m_res(R) / ref.HEADROOM)
    print(f"D={n_cols}: {lower} <= {inside} <= {upper}; from M_ref {from_m_ref}, twice as wide {twice}")
    assert 1000 < lower <= inside <= upper
    assert from_m_ref < 0.5 * lower and twice > 1.5 * upper
    # the band of these widths: e0 = 3.51e-4 S M at 1024 columns, four times the M here
    if n_cols == 1024:
        s, e0, _ = ref.band(n_cols, R)
        assert abs(e0 / (s * ref.m_res(R)) - 3.51e-4) < 0.02e-4
