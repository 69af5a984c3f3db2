"""Cases of the assigner's tests (dc_hip_assign_*, dc_hip_assigner_*, `clustering assign`):
tests/test_assign_cases.py checks their premises in numpy, tests/test_gpu_assign.py and tests/test_gpu_cli_assign.py run
them on the device.  Importing this module needs neither a GPU nor torch.

Every reference but the lattice is referenceref's three blobs, at every width: a reference of the resident handles' tests,
with their gate cases (inside the 4 x extent, beyond it)."""
import numpy as np

import referenceref as ref
import refmath

F32 = np.float32
NARROW, WIDE = (1, 3, 10, 64), (65, 100, 256)
N_REF, MAX_BATCH = 1500, 300
BATCHES = (1, 33, 300, 1100)   # in sequence on ONE handle; the last is chunked (300, 300, 300, 200)


def reference(D, n=N_REF):
    return ref.reference_rows(D, n)


def radius(D):
    """r^2 = 0.9 of the mean squared distance inside a blob (2 D sigma^2): some tens to some hundreds of neighbours at
    every width -- at 256 columns the squared distances of a blob lie within a few percent of their mean, and
    referenceref's radius (0.64 of it) would leave every frame alone"""
    return float(ref.SIGMA * np.sqrt(0.9 * 2.0 * D))


def states_of(n, seed=5):
    """a state per reference row, 0 (unassigned) among them"""
    return np.random.default_rng(seed).integers(0, 6, n).astype(np.int32)


def batch(R, n_q, seed=31):
    return ref.ordinary_batch(R, n_q, seed)


# ---- the lattice: every population a query can have ------------------------------------------------------------------------------
LATTICE_N, LATTICE_R = 1500, 700.5
LATTICE_LOW_MAX_POP = 1000   # a scale below the lattice's own: queries of 1 001 .. 1 401 neighbours then have negative free energies


def lattice():
    """(Q, R): R the 1 500 points 0, 1, ..., 1 499 on a line, Q at -r + j + 0.5 = j - 700 for j = -1 .. 1 400.  Query j has
    min(j + 1, 1 401) reference points strictly within r = 700.5: every population 0 .. 1 401 occurs.  The reference's own
    largest population is 1 401 as well (an inner point, itself included), so on the reference's own scale no query
    exceeds max_pop: the test runs the case a second time on the scale LATTICE_LOW_MAX_POP."""
    R = np.arange(LATTICE_N, dtype=np.float32).reshape(-1, 1)
    j = np.arange(-1, 1401, dtype=np.float64)
    Q = (-LATTICE_R + j + 0.5).astype(np.float32).reshape(-1, 1)
    return np.ascontiguousarray(Q), np.ascontiguousarray(R)


def lattice_populations(Q, R):
    r2 = F32(LATTICE_R) * F32(LATTICE_R)
    d = (Q[:, None, 0] - R[None, :, 0]).astype(F32)
    return ((d * d).astype(F32) < r2).sum(axis=1)


# ---- the gate -------------------------------------------------------------------------------------------------------------------
def far_batch(R, n_q, seed=31):
    """an ordinary batch whose rows ref.headroom_rows(n_q) sit beyond every blob (population 0) and inside the handles'
    4 x extent: the matrix cores answer it"""
    return ref.headroom_batch(R, n_q, seed)


def flagged_batch(R, n_q, seed=31):
    """an ordinary batch with a NaN in row 5 and row n_q // 2 beyond the 4 x extent: the direct kernels answer it
    (answered == 2)"""
    Q = ref.beyond_batch(R, n_q, seed)
    Q[5, R.shape[1] - 1] = np.nan
    return Q


# ---- ties, on the k / 8 lattice (every difference and squared distance exact) ------------------------------------------------------
TIE_RADIUS = 0.2
TIE_ROWS = (3, 20)   # the duplicate reference rows, with different states


def tie_case():
    """(Q, R, states): a reference of 33 rows in 3 columns.  Rows 3 and 20 are the SAME point, the origin, with states 5
    and 6; rows 4 .. 9 its six neighbours at 1 / 8 along the axes; the other rows lie far apart from everything.  At
    r = 0.2 the origin holds 8 rows (itself twice and the six), a neighbour 7: the duplicates are the rows of the largest
    population, free energy 0.
    Query 0 is the origin: population 8 = max_pop, free energy 0 -- EQUAL to the duplicates', lower than nobody's: hd is
    "none", the state comes through nn, and nn is tied between rows 3 and 20 at d2 = 0.
    Query 1 is (1 / 16, 0, 0): 1 / 16 from rows 3, 20 and 4 -- a tie of three --, population 8 again.
    Both get the state of row 3."""
    R = np.zeros((33, 3), np.float32)
    far = 0
    for i in range(33):
        if i in TIE_ROWS:
            continue
        if 4 <= i <= 9:
            k = i - 4
            R[i, k // 2] = F32(0.125) * (1 if k % 2 == 0 else -1)
        else:
            far += 1
            R[i] = (8.0 * far, 8.0, -8.0)
    states = (np.arange(33) % 4 + 1).astype(np.int32)
    states[TIE_ROWS[0]], states[TIE_ROWS[1]] = 5, 6
    Q = np.array([[0.0, 0.0, 0.0], [0.0625, 0.0, 0.0]], np.float32)
    return Q, np.ascontiguousarray(R), states


def canonical_d2(Q, R):
    """canonical d2 of every (query, reference) pair, float32 [n_q, n_ref] (refmath)"""
    both = np.concatenate([Q, R]).astype(np.float32)
    return refmath.d2_matrix(both)[:len(Q), len(Q):]
