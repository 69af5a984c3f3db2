"""CPU: the premises of the assigner's cases (tests/assignref.py), in numpy -- that the lattice holds every population, that
the tie cases tie in canonical d2, that the far queries are empty and inside the gate and the flagged ones outside it."""
import numpy as np
import pytest

import assignref as cases
import referenceref as ref

F32 = np.float32


def test_the_lattice_holds_every_population():
    Q, R = cases.lattice()
    assert R.shape == (1500, 1) and (np.diff(R[:, 0]) == 1).all()
    j = np.arange(-1, 1401)
    assert (Q[:, 0] == (-cases.LATTICE_R + j + 0.5)).all(), "the query positions are exact floats"
    pops = cases.lattice_populations(Q, R)
    assert (pops == np.minimum(j + 1, 1401)).all()
    assert set(range(0, 1401)) <= set(pops.tolist()), "every population 0 .. 1 400 occurs"
    # the reference's own largest population (self included) is 1 401: on its own scale no query exceeds max_pop ...
    own = cases.lattice_populations(R, R)
    assert own.max() == 1401 and pops.max() == 1401
    # ... on the lower scale of the second run some do
    assert (pops > cases.LATTICE_LOW_MAX_POP).sum() == 401 and (pops == 0).sum() == 1
    # the farthest query is inside the handle's 4 x extent
    assert ref.norms(Q, R).max() < ref.m_res(R)


def test_the_tie_case_ties_in_canonical_d2():
    Q, R, states = cases.tie_case()
    a, b = cases.TIE_ROWS
    assert (R[a] == R[b]).all() and states[a] != states[b] and 0 not in (states[a], states[b])
    d2 = cases.canonical_d2(Q, R)
    r2 = F32(cases.TIE_RADIUS) * F32(cases.TIE_RADIUS)
    # query 0: d2 = 0 to both duplicates and to nothing else; query 1: three rows at the same least d2
    assert d2[0, a] == d2[0, b] == 0 and (np.delete(d2[0], [a, b]) > 0).all()
    least = d2[1].min()
    assert sorted(np.flatnonzero(d2[1] == least).tolist()) == [3, 4, 20] and least == F32(1.0 / 256.0)
    # populations: both queries hold what the duplicates hold, the largest population of the reference
    pops_ref = (cases.canonical_d2(R, R) < r2).sum(axis=1)
    pops_q = (d2 < r2).sum(axis=1)
    assert pops_ref.max() == 8 and sorted(np.flatnonzero(pops_ref == 8).tolist()) == [a, b]
    assert (pops_q == 8).all(), "equal free energies: no reference row is lower, hd is none"
    # no pair sits near the radius (the nearest are 3 / 16 = 0.1875 and 1 / 4 apart)
    assert not ((d2 > 0.9 * r2) & (d2 < 1.1 * r2)).any()


@pytest.mark.parametrize("D", cases.NARROW + cases.WIDE)
def test_far_queries_are_empty_and_inside_the_gate_and_flagged_ones_outside(D):
    R = cases.reference(D)
    assert R.shape == (cases.N_REF, D)
    r2 = float(F32(cases.radius(D)) * F32(cases.radius(D)))
    m_res = float(ref.m_res(R))
    Q = cases.far_batch(R, 300)
    rows = ref.headroom_rows(300)
    d2 = ref.d2_exact(Q[rows], R)
    assert (d2.min(axis=1) > 1.2 * r2).all(), "population 0, with a margin no rounding closes"
    assert (ref.norms(Q, R) < 0.75 * m_res).all(), "inside the 4 x extent"
    assert np.median((ref.d2_exact(Q, R) < r2).sum(axis=1)) >= 40, "the batch is not empty: tens of neighbours and more"
    F = cases.flagged_batch(R, 300)
    n = ref.norms(F, R)
    assert np.isnan(F[5]).any() and n[150] > 1.5 * m_res
    assert np.isfinite(np.delete(F, 5, axis=0)).all() and (np.delete(n, [5, 150]) < 0.75 * m_res).all()


def test_states_hold_the_unassigned_state():
    s = cases.states_of(cases.N_REF)
    assert s.dtype == np.int32 and (s == 0).any() and (s > 0).any()
