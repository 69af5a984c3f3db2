"""Cases of the pruned population sweep against a reference (variant="cross_pruned"), shared by the GPU tests
(tests/test_gpu_cross_pruned.py, and its child processes of the other summation orders) and by the CPU test of their
premises (tests/test_cross_pruned_cases.py).  Nothing here needs a GPU or torch."""
import numpy as np

from crossref import F32, square
from prunedref import radius_for

STEP = F32(2.0 ** -3)   # lattice spacing of the boundary cases: coordinates k / 8, squared distances m / 64, all exact


# ---- case 2: who answered ---------------------------------------------------------------------------------------------
BLOB_R, BLOB_SEP, BLOB_SIGMA, BLOB_ROWS = 0.2, 100.0, 0.05, 1024


def two_blobs(D=10, seed=21):
    """R: two blobs of 1024 frames, sigma 0.05, 100 apart in column 0; Q: 1024 frames of the first blob only"""
    rng = np.random.default_rng(seed)
    a = (rng.normal(size=(BLOB_ROWS, D)) * BLOB_SIGMA).astype(np.float32)
    b = (rng.normal(size=(BLOB_ROWS, D)) * BLOB_SIGMA).astype(np.float32)
    b[:, 0] += F32(BLOB_SEP)
    R = np.vstack([a, b])[rng.permutation(2 * BLOB_ROWS)]
    Q = (rng.normal(size=(BLOB_ROWS, D)) * BLOB_SIGMA).astype(np.float32)
    return np.ascontiguousarray(Q), np.ascontiguousarray(R)


def shifted(Q):
    """the queries moved between the blobs: +50 in column 0"""
    S = Q.copy()
    S[:, 0] += F32(BLOB_SEP / 2)
    return S


# ---- case 3: boundary lattice -------------------------------------------------------------------------------------------
def lattice_points(x_idx, y_idx, D, fill=0.5):
    """the points (x / 8, y / 8, fill, fill, ...) for every x in x_idx, y in y_idx"""
    xs, ys = np.meshgrid(np.asarray(x_idx), np.asarray(y_idx), indexing="ij")
    c = np.full((xs.size, D), F32(fill), dtype=np.float32)
    c[:, 0] = xs.ravel().astype(np.float32) * STEP
    if D > 1:
        c[:, 1] = ys.ravel().astype(np.float32) * STEP
    return c


def lattice_radii():
    """(g, [r_at, r_above, r_below]): the smallest lattice distance g / 8 for which r^2 = g^2 / 64, the float above it
    and the float below it are all squares of floats -- the library squares its radii, so only such a level can be
    approached from both sides (g = 23, as prunedref.GAP_PLANE found for the self sweeps; no level k / 64 with k a sum
    of two non-zero squares below 19^2 + 19^2 has all three)"""
    for g in range(1, 64):
        r2 = F32(g * g) * STEP * STEP
        trio = [radius_for(r2), radius_for(np.nextafter(r2, F32(np.inf))), radius_for(np.nextafter(r2, F32(0.0)))]
        if all(r is not None for r in trio):
            return g, trio
    raise AssertionError("no lattice level with reachable neighbours")


def lattice_sets(D, g, seed=5):
    """Q and R on overlapping pieces of the lattice (several tiles each, shuffled): many pairs exactly g / 8 apart"""
    rng = np.random.default_rng(seed)
    R = lattice_points(range(0, 2 * g + 6), range(0, 12), D)
    Q = lattice_points(range(g, 3 * g + 3), range(3, 15), D)
    return Q[rng.permutation(len(Q))], R[rng.permutation(len(R))]


def lattice_gap_sets(D, g):
    """one tile each (32 rows: a tile's box is the set's box whatever the order): R spans x = 0..3, Q x = g+3..g+6, the
    same y -- the boxes are EXACTLY g / 8 apart in column 0, and the facing columns hold pairs at exactly that d"""
    R = lattice_points(range(0, 4), range(0, 8), D)
    Q = lattice_points(range(g + 3, g + 7), range(0, 8), D)
    return Q, R


def box_gap(Q, R):
    """distance of the bounding boxes of Q and R in the (col 0, col 1) plane, in float as box_gap2 forms it"""
    def ext(c, k):
        v = c[:, k] if c.shape[1] > k else np.zeros(len(c), np.float32)
        return F32(v.min()), F32(v.max())
    d = []
    for k in (0, 1):
        (ql, qh), (rl, rh) = ext(Q, k), ext(R, k)
        d.append(max(F32(0.0), F32(ql - rh), F32(rl - qh)))
    return F32(np.sqrt(np.float64(F32(d[0] * d[0] + d[1] * d[1]))))


# ---- case 9: degenerate grids -------------------------------------------------------------------------------------------
DISJOINT_R = 0.2


def degenerate_cases():
    """(name, Q, R, radii)"""
    rng = np.random.default_rng(9)
    out = []
    # all of R in one point
    R = np.tile((rng.normal(size=(1, 10)) * 0.1).astype(np.float32), (100, 1))
    Q = (R[0] + rng.normal(size=(300, 10)) * 0.08).astype(np.float32)
    Q[::9] = R[0]
    out.append(("one point", Q, R, [0.2, 0.1]))
    # every row equal in columns 0/1, spread in column 2: every box is one point of the plane, every gap 0
    R = np.zeros((700, 3), np.float32)
    R[:, :2] = F32(0.25)
    R[:, 2] = rng.normal(size=700).astype(np.float32)
    Q = np.zeros((333, 3), np.float32)
    Q[:, :2] = F32(0.25)
    Q[:, 2] = rng.normal(size=333).astype(np.float32)
    out.append(("one column", Q, R, [0.2, 0.05]))
    # the bounding boxes of Q and R do not meet but are closer than r
    R = rng.uniform(0.0, 1.0, size=(900, 10)).astype(np.float32) * F32(0.3)
    R[:, 0] = rng.uniform(0.0, 1.0, size=900).astype(np.float32)
    Q = R[:400].copy()
    Q[:, 0] = rng.uniform(1.05, 2.0, size=400).astype(np.float32)
    Q[:, 2:] += (rng.normal(size=(400, 8)) * 0.01).astype(np.float32)
    out.append(("disjoint boxes", Q, R, [DISJOINT_R]))
    # one query, 64 and 65 references (two full tiles; one row into the third)
    base = (rng.normal(size=(65, 10)) * 0.1).astype(np.float32)
    out.append(("one query, 64", base[:1].copy(), base[:64].copy(), [0.3, 0.2]))
    out.append(("one query, 65", base[:1].copy(), base.copy(), [0.3, 0.2]))
    return out
