"""CPU: the premises of tests/test_gpu_wide_reference.py, on the cases of tests/referencewideref.py, in float64 with room
against rounding: what an "ordinary" batch, a batch "inside the headroom, outside the extent" and a batch "beyond the
headroom" are, that the reference-only grid order is a pair of permutations which clamps the queries, and that the pruning
case leaves at least a third of the block pairs out under that order."""
import numpy as np
import pytest

import crosswidennpruneref as nnref
import crosswidepruneref as pr
import crosswideref as cw
import referencewideref as ref


@pytest.mark.parametrize("n_r,n_cols", ref.REFERENCES)
def test_the_three_kinds_of_batch(n_r, n_cols):
    R = ref.reference_rows(n_r, n_cols)
    m = ref.m_ref(R)
    assert R.shape == (n_r, n_cols) and m > 0
    for k, n_q in enumerate(ref.BATCHES):
        Q = ref.ordinary_batch(R, n_q, seed=40 + k)
        assert Q.shape == (n_q, n_cols) and np.isfinite(Q).all()
        assert ref.norms2(Q, R).max() < 0.9 * m, "ordinary: well inside the reference's own extent"
    Q = ref.headroom_batch(R, 300)
    n2 = ref.norms2(Q, R)
    assert 1.5 * m <= n2.max() <= 2.7 * m, "inside the headroom: below M_res = 4 M_ref with room, above M_ref with room"
    far = n2 > 1.5 * m
    assert 1 <= far.sum() <= 4 and ref.outside_box(Q, R)[far].all(), "... and outside the reference's box in columns 0 / 1"
    lo, hi = R[:, :2].astype(np.float64).min(axis=0), R[:, :2].astype(np.float64).max(axis=0)
    edge = np.minimum(np.abs(Q[far, :2] - lo), np.abs(Q[far, :2] - hi)).min()
    assert edge > 1e-3 * (hi - lo).max(), "by more than rounding"
    Q = ref.beyond_batch(R, 300)
    n2 = ref.norms2(Q, R)
    assert n2.max() >= 6.0 * m and (n2 >= 6.0 * m).sum() == 1 and np.isfinite(Q).all(), "beyond the headroom: one finite row"
    assert np.sort(n2)[-2] < 0.9 * m


def test_the_reference_only_order_clamps_the_queries():
    R = ref.reference_rows(1500, 100)
    Q = ref.headroom_batch(R, 300)
    perm_q, perm_r = ref.reference_order(Q, R)
    assert sorted(perm_q.tolist()) == list(range(300)) and sorted(perm_r.tolist()) == list(range(1500))
    # the reference's order does not depend on the batch; the joint order of the pruned cross sweep does
    for other in (ref.ordinary_batch(R, 129), ref.beyond_batch(R, 300)):
        assert (ref.reference_order(other, R)[1] == perm_r).all()
    assert (pr.joint_order(Q, R)[1] != perm_r).any()
    # a batch inside the reference's box gets the order the joint grid of the two would give it whenever the joint extent is the reference's
    inside = R[100:400].copy()
    assert not ref.outside_box(inside, R).any()
    jq, jr = pr.joint_order(inside, R)
    rq, rr = ref.reference_order(inside, R)
    assert (jq == rq).all() and (jr == rr).all()
    # the boxes of the clamped rows are true boxes: formed from their own floats, they reach beyond the reference's extent
    boxes = pr.block_boxes(Q, perm_q)
    lo, hi = R[:, :2].min(axis=0), R[:, :2].max(axis=0)
    assert (boxes[:, 0].min() < lo[0]) and (boxes[:, 1].max() > hi[0])


def test_the_pruning_case_leaves_a_third_of_the_block_pairs_out():
    Q, R, fe_q, fe_r = ref.prune_case()
    assert not ref.outside_box(Q, R).all()
    perm_q, perm_r = ref.reference_order(Q, R)
    g = pr.gaps(Q, R, perm_q, perm_r)
    radii = pr.radii_for(Q.shape[1], 3)
    lo, hi = pr.tile_bounds(Q, R, perm_q, perm_r, radii)
    assert 0 < lo <= hi <= 16 * g.size * 2 // 3, (lo, hi, g.size)
    lo, hi = nnref.tile_bounds(Q, R, fe_q, fe_r, perm_q, perm_r)
    assert 0 < lo <= hi <= 16 * g.size * 2 // 3, (lo, hi, g.size)


def test_the_edge_cases_are_what_they_say():
    R = ref.reference_rows(1500, 100)
    assert ref.m_ref(R[:1]) == 0.0, "a reference of one row: every other point is beyond its headroom"
    Q = ref.ordinary_batch(R[:129], 300)
    assert ref.norms2(Q, R[:129]).max() < 0.9 * ref.m_ref(R[:129])
    assert ref.norms2(R, R).max() == ref.m_ref(R) < ref.HEADROOM * ref.m_ref(R), "the batch that is the reference is inside"
    Qb, Rb, r, groups = cw.boundary_sets(300, 1500, 100)
    assert ref.norms2(Qb, Rb).max() < 3.9 * ref.m_ref(Rb), "the boundary batch runs on the matrix cores"
