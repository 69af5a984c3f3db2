"""CPU: the premises of the resident reference's GPU cases (tests/test_gpu_reference.py), checked in numpy from
tests/referenceref.py -- each boundary case really has pairs at d2 == r^2 and one ulp either side, each tie really ties,
each "beyond" row really lies beyond 4 M_ref in float32 as the gate forms it, each "inside the headroom" row really lies
below it and outside the reference's box, and the restated orders are orders."""
import numpy as np
import pytest

import crossbigref as big
import referenceref as ref

F32 = np.float32


@pytest.mark.parametrize("D", ref.WIDTHS)
def test_ordinary_headroom_and_beyond_batches_lie_where_they_should(D):
    R = ref.reference_rows(D)
    m, m4 = ref.m_ref(R), ref.m_res(R)
    assert 0 < m and np.isfinite(m4) and m4 == F32(4.0) * m
    for k, n_q in enumerate(ref.BATCHES):
        assert (ref.norms(ref.ordinary_batch(R, n_q, seed=40 + k), R) <= m4).all(), "an ordinary batch passes the gate"
    H = ref.headroom_batch(R, 300)
    moved = ref.headroom_rows(300)
    assert len(moved) == 4 and ref.outside_box(H, R)[moved].all() and (ref.norms(H, R) <= m4).all(), "outside the box, below 4 M_ref"
    assert (ref.norms(H[moved], R) > F32(2.0) * m).all(), "... and well beyond the reference's own extent"
    B = ref.beyond_batch(R, 300)
    n = ref.norms(B, R)
    assert (n > m4).sum() == 1 and n[150] > m4 and np.isfinite(n).all(), "one finite row beyond 4 M_ref"


def test_the_flawed_references_are_flagged_for_the_reason_named():
    R = ref.reference_rows(10)
    for flaw in ("nan", "inf"):
        assert not np.isfinite(ref.flawed_reference(R, flaw)).all()
    B = ref.flawed_reference(R, "big")
    n = ref.norms(B, B)
    assert np.isfinite(B).all() and (n <= F32(1.0e36)).all(), "no row alone is beyond kNormLimit"
    assert not F32(4.0) * F32(n.max()) <= F32(1.0e36), "four times the largest is"


@pytest.mark.parametrize("D", [3, 10])
def test_the_boundary_case_has_pairs_at_the_level_and_the_radii_straddle_it(D):
    Q, R, (r_at, r_above, r_below) = ref.boundary_case(D)
    d2 = ref.d2_exact(Q, R)
    level = float(F32(r_at) * F32(r_at))
    assert (d2 == level).sum() > 100, "many pairs exactly at r^2"
    assert float(F32(r_above) * F32(r_above)) == float(np.nextafter(F32(level), F32(np.inf)))
    assert float(F32(r_below) * F32(r_below)) == float(np.nextafter(F32(level), F32(0.0)))
    at = (d2 < level).sum()
    assert (d2 < float(F32(r_above) * F32(r_above))).sum() == at + (d2 == level).sum(), "one ulp above takes them in"
    assert (d2 < float(F32(r_below) * F32(r_below))).sum() == at, "strict <: at the level and one ulp below count alike"
    assert (ref.norms(Q, R) <= ref.m_res(R)).all(), "the lattice queries pass the gate"


@pytest.mark.parametrize("D", [3, 10])
def test_the_tie_case_ties(D):
    Q, R, fe_q, fe_r = ref.tie_case(D)
    d2 = ref.d2_exact(Q, R)
    least = d2.min(axis=1)
    ties = (d2 == least[:, None]).sum(axis=1)
    assert (ties[:96] >= 2).all() and (least[:96] == 1.0 / 256.0).all(), "half a step from two reference rows"
    assert (least[96:] == 0.0).all() and (ties[96:128] >= 2).all(), "on a reference row, the first 32 on a row and its copy"
    assert (R[200:232] == R[0:32]).all()
    assert all((fe_r == f).any() for f in np.unique(fe_q)[:-1]), "query levels that reference rows share: equal is not lower"
    assert (ref.norms(Q, R) <= ref.m_res(R)).all()


@pytest.mark.parametrize("D", [1, 3, 10])
def test_the_restated_orders_are_orders_and_clamp_outside_rows(D):
    R = ref.reference_rows(D)
    Q = ref.headroom_batch(R, 300)
    fe_r = ref.fe_pair(300, len(R))[1]
    for which, frames in ((0, big.POP_CELL), (1, big.NN_CELL)):
        for fe in (None, fe_r):
            perm_q, perm_r = ref.orders(Q, R, which, fe)
            assert sorted(perm_q.tolist()) == list(range(len(Q))) and sorted(perm_r.tolist()) == list(range(len(R)))
        lo0, lo1, cell, ny = ref.grid(R, frames)
        kq, kr = ref.cell_keys(Q, R, frames), ref.cell_keys(R, R, frames)
        inside = ~ref.outside_box(Q, R)
        assert 0 <= kq.min() and kq[inside].max() <= kr.max() and kq.max() <= 4000 * ny + ny - 1, "rows outside the extent are clamped"
        assert kr.max() < (1 << big.cell_key_bits(len(R), frames)), "the sort sees every bit of the keys"
    boxes = ref.tile_boxes(R, ref.orders(Q, R, 0)[1])
    assert len(boxes) == (len(R) + 31) // 32 and (boxes[:, 0] <= boxes[:, 1]).all()
