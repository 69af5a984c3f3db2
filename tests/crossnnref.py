"""Built cases of the pruned neighbour sweep against a reference (nearest_reference(..., pruned=True)), shared by the
GPU tests (tests/test_gpu_cross_nn_pruned.py and its child processes) and by the CPU test of their premises
(tests/test_cross_nn_pruned_cases.py).  Nothing here needs a GPU or torch."""
import numpy as np

import crossprunedref as cp
from crossref import F32

TQ_BUILT = 6   # most query tiles per wave of any built instance (tq_nn: 6 for one or two MFMAs per chain, else 4 or 2)


# ---- case 2: who answered ---------------------------------------------------------------------------------------------
def who_answered(seed=31):
    """crossprunedref.two_blobs with free energies assigned directly: fe_ref uniform in [0, 1), fe_q in [0.5, 1.5)"""
    Q, R = cp.two_blobs()
    rng = np.random.default_rng(seed)
    fe_r = rng.uniform(0.0, 1.0, len(R)).astype(np.float32)
    fe_q = rng.uniform(0.5, 1.5, len(Q)).astype(np.float32)
    return Q, R, fe_q, fe_r


def own_blob(R):
    """mask of the reference frames of the queries' blob (the one at the origin)"""
    return R[:, 0] < F32(cp.BLOB_SEP / 2)


# ---- case 3 (a): equal d2 in two reference tiles on opposite sides, met in different rings ---------------------------
TIE_D2 = F32(25.0)          # squared distance of the tie: 5 = |(-5, 0)| = |(3, 4)| = |(3, -4)|
NN_CELL_FRAMES = 128.0      # dc_mfma_kernels.hpp kNnCellFrames: reference frames per cell of the neighbour sweep's grid
TIE_ROWS = 2048


def tie_sets(D):
    """On the k / 8 lattice (exact arithmetic).  Q: 32 rows on the point (0, 0).  Reference rows 0..31, the FAR rows,
    lie on (-5, 0); rows 32..63, the NEAR rows, on (3, 4) and (3, -4): all 64 at exactly d2 = 25 from every query.  Rows
    64..2047 are filler of higher index, farther than that (x >= 5.125), on the lattice of [5.125, 7.5] x [-4, 4].
    What the filler is for: the common box is 12.5 x 8 and holds 2048 reference rows, so the grid's cell edge is
    sqrt(12.5 * 8 * 128 / 2048) = 2.5 exactly and the sweep's first ring ends at cell^2 = 6.25 -- below the box gap of
    every reference tile (>= 9), so it is empty and the next ring ends at 4 * 6.25 = 25 EXACTLY.  The far rows are the
    only ones in the first column of cells, hence tile 0 of the order, a box of one point whose gap^2 is 25: not inside
    that ring.  The near rows are the only ones in their column, hence tile 1, box gap^2 9: inside it.  After that ring
    every query's incumbent is d2 = 25 with an index >= 32, equal to the ring's end: only the settle margin sends the
    wave into the ring that holds the far tile and index 0."""
    def rows(x, y):
        x, y = np.atleast_1d(np.asarray(x, dtype=np.float32)), np.atleast_1d(np.asarray(y, dtype=np.float32))
        c = np.full((len(x), D), F32(0.5), dtype=np.float32)
        c[:, 0], c[:, 1] = x, y
        return c
    xs, ys = np.meshgrid(np.arange(41, 61) * cp.STEP, np.arange(-32, 33) * cp.STEP, indexing="ij")
    fill = np.resize(np.arange(xs.size), TIE_ROWS - 64)
    R = np.vstack([rows(np.full(32, -5.0), np.zeros(32)), rows(np.full(16, 3.0), np.full(16, 4.0)),
                   rows(np.full(16, 3.0), np.full(16, -4.0)), rows(xs.ravel()[fill], ys.ravel()[fill])])
    return rows(np.zeros(32), np.zeros(32)), R


def cell_order(Q, R, frames_per_cell=NN_CELL_FRAMES):
    """the grid and the reference order of the pruned sweeps against a reference, restated (dc_prep.hpp against_grid,
    against_key_kernel; dc_mfma_kernels.hpp auto_cell): -> (cell edge, stable order of R by serpentine cell key)"""
    both = np.vstack([Q, R])
    lo0, lo1 = F32(both[:, 0].min()), F32(both[:, 1].min())
    e0, e1 = F32(both[:, 0].max() - lo0), F32(both[:, 1].max() - lo1)
    f = float(frames_per_cell) / len(R)
    auto = np.sqrt(float(e0) * float(e1) * f) if e0 > 0 and e1 > 0 else (float(e0) + float(e1)) * f
    cell = max(F32(auto), F32(max(e0, e1) / F32(4000.0)))
    ny = int(min(F32(e1 / cell), F32(4000.0))) + 1
    bx = np.minimum(np.maximum((R[:, 0] - lo0) / cell, F32(0)), F32(4000)).astype(np.int64)
    by = np.minimum(np.minimum(np.maximum((R[:, 1] - lo1) / cell, F32(0)), F32(4000)).astype(np.int64), ny - 1)
    key = bx * ny + np.where(bx & 1, ny - 1 - by, by)
    return cell, np.argsort(key, kind="stable")


def tie_fe(n_q, n_r):
    """free energies that put the tie inside the hd set: references 0..2 are not lower than the queries, all others are"""
    fe_r = (np.arange(n_r) % 7).astype(np.float32) / F32(8.0)
    fe_r[:3] = F32(2.0)
    return np.full(n_q, F32(1.0)), fe_r


# ---- case 5: a lower frame only far away ------------------------------------------------------------------------------
def far_lower(seed=5, D=10, n=600):
    """R: blob 1 at the origin (rows with fe in [1, 2)) and blob 2 100 away in column 0 (fe in [3, 4), but ONE frame of it
    at 0.25).  Q: frames of blob 1; the first 40 have fe_q = 0.5 -- lower than all of blob 1, not lower than that one frame
    -- the others fe_q = 2.5 (all of blob 1 is lower, and that frame)."""
    rng = np.random.default_rng(seed)
    a = (rng.normal(size=(n, D)) * 0.05).astype(np.float32)
    b = (rng.normal(size=(n, D)) * 0.05).astype(np.float32)
    b[:, 0] += F32(100.0)
    R = np.vstack([a, b])
    fe_r = np.concatenate([rng.uniform(1.0, 2.0, n), rng.uniform(3.0, 4.0, n)]).astype(np.float32)
    special = n + 17
    fe_r[special] = F32(0.25)
    perm = rng.permutation(2 * n)
    R, fe_r = np.ascontiguousarray(R[perm]), np.ascontiguousarray(fe_r[perm])
    special = int(np.flatnonzero(perm == special)[0])
    Q = (rng.normal(size=(300, D)) * 0.05).astype(np.float32)
    fe_q = np.full(300, F32(2.5))
    fe_q[:40] = F32(0.5)
    return Q, R, fe_q, fe_r, special
