"""Case generators and the numpy restatement of the resident reference's grid and orders (dc_hip_reference_*, rows of
1..64 columns): tests/test_reference_cases.py checks their premises on the CPU,
tests/test_gpu_reference.py runs them on the device.  Importing this module needs neither a GPU nor torch.

What differs from the per-call pruned cross sweeps (crossbigref): origin, extent and grid come from the REFERENCE alone.
The origin is its column mean, the extent M_res = 4 M_ref (M_ref the largest |x - mean|^2 of the reference), the grid its
extent in columns 0 / 1 -- a query outside it is clamped into an edge cell."""
import numpy as np

import crossbigref as big
import crossprunedref as cp
from crossref import F32

HEADROOM = 4.0   # M_res / M_ref
N_REF, MAX_BATCH = 1500, 1100
# the ends, the instance classes of crossbigref.CLASS_WIDTHS (NM = 1, 2, 4, 5), and 7: odd, so the gate reads a row word
# by word (1 and 3 are odd as well; 7 is the odd width with more than one pair's worth of columns)
WIDTHS = (1, 3, 7, 10, 16, 24, 64)
BATCHES = (300, 1, 33, 1100, 191, 192, 193)   # 192 rows = 6 query tiles: one wave's share at NM <= 2
SIGMA, SEP = 0.25, 4.0


# ---- data -------------------------------------------------------------------------------------------------------------------
def blobs(n, D, seed):
    """three well-separated blobs: sigma 0.25 in every column, centres (0, 0), (4, 0), (0, 4) in columns 0 / 1 (two blobs on
    a line at D = 1), rows shuffled"""
    rng = np.random.default_rng(seed)
    X = (rng.normal(size=(n, D)) * SIGMA).astype(np.float32)
    which = rng.integers(0, 3, n)
    X[:, 0] += np.where(which == 1, F32(SEP), F32(0.0))
    if D > 1:
        X[:, 1] += np.where(which == 2, F32(SEP), F32(0.0))
    return np.ascontiguousarray(X)


def reference_rows(D, n=N_REF):
    return blobs(n, D, seed=7)


def radius(D):
    """a radius that gives a blob frame some tens of neighbours: 0.8 of the typical distance inside a blob"""
    return float(0.8 * SIGMA * np.sqrt(2.0 * D))


def radii(D, n):
    """n radii around radius(D), not ascending"""
    return [radius(D) * f for f in (1.0, 0.6, 1.2, 0.9, 0.5, 1.1, 0.7, 0.8, 1.15)[:n]]


def max_radius(D):
    return radius(D) * 1.2


def fe_pair(n_q, n_r, seed=17):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 1.5, n_q).astype(np.float32), rng.uniform(0.0, 1.0, n_r).astype(np.float32)


# ---- the statistics of the reference alone, as the device forms them ----------------------------------------------------------
def means(R):
    """the resident origin: double column sums, divided, rounded to float"""
    return (R.astype(np.float64).sum(axis=0) / len(R)).astype(F32)


def norms(X, R):
    """fl32(|x - mean(R)|^2) of every row of X as rowstats_kernel and the gate form it: the differences in float, their
    squares summed in double in column order, rounded once"""
    d = (X - means(R)).astype(F32).astype(np.float64)
    acc = np.zeros(len(X))
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(X.shape[1]):
            acc = acc + d[:, k] * d[:, k]
        return acc.astype(F32)


def m_ref(R):
    return F32(norms(R, R).max())


def m_res(R):
    return F32(HEADROOM) * m_ref(R)


def outside_box(Q, R):
    """rows of Q whose column 0 or column 1 lies outside the reference's extent"""
    k = min(2, R.shape[1])
    lo, hi = R[:, :k].min(axis=0), R[:, :k].max(axis=0)
    return ((Q[:, :k] < lo) | (Q[:, :k] > hi)).any(axis=1)


# ---- batches ------------------------------------------------------------------------------------------------------------------
def ordinary_batch(R, n_q, seed=31):
    """n_q frames of the reference's distribution, none of them a reference row"""
    return blobs(n_q, R.shape[1], seed=1000 + seed)


def _moved(R, Q, rows, factor, planar):
    """Q with `rows` put at mean + d, |d|^2 = factor M_ref; planar: d in the (column 0, column 1) plane, a corner each
    (column 0 alone at D = 1); otherwise d along the last column"""
    Q, mu, m, D = Q.copy(), means(R).astype(np.float64), float(m_ref(R)), R.shape[1]
    for k, i in enumerate(rows):
        d = np.zeros(D)
        if planar and D > 1:
            d[0] = np.sqrt(0.5 * factor * m) * (1 if k & 1 else -1)
            d[1] = np.sqrt(0.5 * factor * m) * (1 if k & 2 else -1)
        elif planar:
            d[0] = np.sqrt(factor * m) * (1 if k & 1 else -1)
        else:
            d[D - 1] = np.sqrt(factor * m)
        Q[i] = (mu + d).astype(F32)
    return np.ascontiguousarray(Q)


def headroom_rows(n_q):
    """the rows headroom_batch moves"""
    return sorted(set([0, n_q // 3, n_q // 2, n_q - 1])) if n_q >= 4 else [0]


def headroom_batch(R, n_q, seed=31):
    """inside the headroom, outside the extent: an ordinary batch with a few rows at |x'|^2 = 2.2 M_ref on the diagonals of
    the (column 0, column 1) plane -- each beyond the reference's box in both columns (|x_k - mean_k| <= sqrt(M_ref) for
    every reference row, these sit at sqrt(1.1 M_ref))"""
    return _moved(R, ordinary_batch(R, n_q, seed), headroom_rows(n_q), 2.2, True)


def beyond_batch(R, n_q, seed=31):
    """beyond the headroom: an ordinary batch with one finite row at |x'|^2 = 7 M_ref"""
    return _moved(R, ordinary_batch(R, n_q, seed), [n_q // 2], 7.0, False)


def flawed_reference(R, flaw):
    """a reference the open call flags: a NaN, an inf, or one finite row whose |x - mean|^2 stays below kNormLimit = 1e36
    while four times it does not"""
    R = R.copy()
    R[7, 0] = {"nan": np.nan, "inf": np.inf, "big": F32(6.0e17)}[flaw]
    return np.ascontiguousarray(R)


# ---- boundaries and ties, on the k / 8 lattice (every coordinate, difference and squared distance exact) -----------------------
def boundary_case(D):
    """(Q, R, [r_at, r_above, r_below]): crossprunedref's lattice with many pairs exactly g / 8 apart, and the three radii
    whose squares are that level, the float above it and the float below it"""
    g, trio = cp.lattice_radii()
    Q, R = cp.lattice_sets(D, g)
    return Q, R, trio


def tie_case(D):
    """(Q, R, fe_q, fe_r).  R: the lattice points of a 24 x 12 patch in shuffled order, with rows 200..231 overwritten by
    copies of rows 0..31 (duplicates: the lower row must win).  Q: 96 queries half a step right of a lattice point -- 1 / 16
    from it and from its right neighbour, d2 = 1 / 256 to both, tied -- and 96 queries ON reference rows 0..95 (d2 = 0 to a
    row and, for the first 32, to its copy).  Free energies from the levels k / 8: a query's level equals that of some
    reference rows, which are then NOT lower."""
    rng = np.random.default_rng(11)
    R = cp.lattice_points(range(0, 24), range(0, 12), D)
    R = R[rng.permutation(len(R))]
    R[200:232] = R[0:32]
    cand = R[32:200].copy()
    cand[:, 0] += cp.STEP / F32(2.0)
    d2 = d2_exact(cand, R)
    tied = cand[(d2 == d2.min(axis=1)[:, None]).sum(axis=1) >= 2][:96]   # (the right neighbour is there: not the patch's edge, not overwritten)
    assert len(tied) == 96
    Q = np.ascontiguousarray(np.vstack([tied, R[0:96]]))
    fe_r = (np.arange(len(R)) % 5).astype(np.float32) / F32(8.0)
    fe_q = ((np.arange(len(Q)) % 5).astype(np.float32) + F32(1.0)) / F32(8.0)
    return Q, np.ascontiguousarray(R), fe_q, fe_r


def d2_exact(Q, R):
    """float64 squared distances; exact for lattice data"""
    q, r = Q.astype(np.float64), R.astype(np.float64)
    return ((q[:, None, :] - r[None, :, :]) ** 2).sum(axis=2)


# ---- the grid of the reference alone and both orders, restated -----------------------------------------------------------------
def _col(X, k):
    return X[:, k] if X.shape[1] > k else np.zeros(len(X), np.float32)


def grid(R, frames):
    """(lo0, lo1, cell edge, ny) of dc_prep.hpp against_grid over header words 8..11 = the extent of R alone"""
    x, y = _col(R, 0), _col(R, 1)
    lo0, lo1 = F32(x.min()), F32(y.min())
    e0, e1 = F32(x.max() - lo0), F32(y.max() - lo1)
    f = float(frames) / len(R)
    auto = np.sqrt(float(e0) * float(e1) * f) if e0 > 0 and e1 > 0 else (float(e0) + float(e1)) * f
    cell = max(F32(auto), F32(max(e0, e1) / F32(4000.0)))
    if not cell > 0:
        cell = F32(1.0)
    ny = int(min(F32(e1 / cell), F32(4000.0))) + 1
    return lo0, lo1, cell, ny


def cell_keys(X, R, frames):
    """the serpentine cell key of every row of X on the reference's grid, a row outside it clamped into an edge cell"""
    lo0, lo1, cell, ny = grid(R, frames)
    bx = np.minimum(np.maximum((_col(X, 0) - lo0) / cell, F32(0)), F32(4000)).astype(np.int64)
    by = np.minimum(np.minimum(np.maximum((_col(X, 1) - lo1) / cell, F32(0)), F32(4000)).astype(np.int64), ny - 1)
    return bx * ny + np.where(bx & 1, ny - 1 - by, by)


def orders(Q, R, which, fe_r=None):
    """(perm_q, perm_r), position -> row, of the population sweep (which = 0: cells of kPopCellFrames) or of the
    neighbour sweep (which = 1: cells of kNnCellFrames, the reference inside a cell by quantised free energy when fe_r is
    given); stable sorts, as the library's radix sort"""
    frames = big.NN_CELL if which else big.POP_CELL
    key_r = cell_keys(R, R, frames)
    bits = big.cell_key_bits(len(R), frames)   # (the sort orders by the low bits it is told of: a key beyond them wraps)
    if which and fe_r is not None:
        cb = big.cell_key_bits(len(R), frames)
        fe_bits = min((24 if cb + 9 <= 24 else 32) - cb, 16)
        lo, hi = F32(fe_r.min()), F32(fe_r.max())
        span = F32(hi - lo)
        u = ((fe_r - lo) / span).astype(np.float32) if span > 0 and np.isfinite(span) else np.zeros(len(R), np.float32)
        u = np.minimum(np.maximum(u, F32(0)), F32(1))
        key_r = (key_r << fe_bits) | (u.astype(np.float64) * float((1 << fe_bits) - 1)).astype(np.int64)
        key_r &= (1 << (bits + fe_bits)) - 1
    else:
        key_r &= (1 << bits) - 1
    return np.argsort(cell_keys(Q, R, frames) & ((1 << bits) - 1), kind="stable"), np.argsort(key_r, kind="stable")


def tile_boxes(X, perm):
    """[T, 4] (lo0, hi0, lo1, hi1) of every 32-row tile of an order, from the rows' own floats (against_rows_kernel)"""
    T = (len(perm) + 31) // 32
    out = np.empty((T, 4), np.float32)
    x, y = _col(X, 0)[perm], _col(X, 1)[perm]
    for t in range(T):
        a, b = x[32 * t:32 * t + 32], y[32 * t:32 * t + 32]
        out[t] = (a.min(), a.max(), b.min(), b.max())
    return out


def pairs_within(Q, R, perm_q, perm_r, r, tq):
    """the count of (query group of tq tiles, reference tile) pairs that hold a pair of rows with float64 d2 < fl32(r * r):
    what a population sweep must at least evaluate, in units of groups x tiles"""
    r2 = float(F32(r) * F32(r))
    d2 = d2_exact(Q[perm_q], R[perm_r]) < r2
    n_g, T_r = -(-len(perm_q) // (32 * tq)), (len(perm_r) + 31) // 32
    count = 0
    for g in range(n_g):
        rows = d2[32 * tq * g:32 * tq * (g + 1)].any(axis=0)
        count += int(np.add.reduceat(rows, np.arange(0, len(perm_r), 32)).astype(bool).sum()) if T_r else 0
    return count
