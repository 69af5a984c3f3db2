"""Case generators and block-pair bounds of the pruned wide cross population sweep's tests (65..256 columns, queries
against a reference): tests/test_cross_wide_pruned_cases.py checks their premises on the CPU with a numpy
joint-grid order, tests/test_gpu_cross_wide_pruned.py runs them on the device and takes both orders from the device
(density.wide_against_pruned_order).  Importing this module needs neither a GPU nor torch.

The pruning check is widepruneref's, on a rectangle: with the boxes of the query blocks and of the reference blocks (128
positions of either order) formed in float64 from the coordinates, every launch evaluates the block pairs with box
gap^2 < r2max and none with gap^2 >= 1.001 r2max, 16 tile pairs each."""
import functools

import numpy as np

import widepruneref as wp
from widepruneref import BLOCK, block_boxes, box_gap2, launch_r2max, n_blocks, radii_for, shares, stretched

F32 = np.float32


def query_blocks(i_from, i_to):
    """blocks of the query order: the range is gathered, so its blocks start at its first row -- ceil((i_to - i_from) / 128),
    whatever blocks of the query ARRAY the range touches"""
    return max(0, (i_to - i_from + BLOCK - 1) // BLOCK)


def joint_order(Q, R, frames_per_cell=BLOCK):
    """both spatial orders as the device builds them, in numpy: ONE cell grid on columns 0 / 1 over the finite entries of
    Q and R together, the cell sized for the REFERENCE's row count, serpentine keys, key 0 for a non-finite row, one stable
    sort per set.  -> (perm_q, perm_r), position -> row of the set"""
    U = np.concatenate([Q[:, :2], R[:, :2]]).astype(np.float64)
    x, y = U[:, 0], U[:, 1]
    fx, fy = np.isfinite(x), np.isfinite(y)
    lo0, hi0 = (x[fx].min(), x[fx].max()) if fx.any() else (0.0, 0.0)
    lo1, hi1 = (y[fy].min(), y[fy].max()) if fy.any() else (0.0, 0.0)
    e0, e1 = hi0 - lo0, hi1 - lo1
    f = frames_per_cell / max(len(R), 1)
    cell = np.sqrt(e0 * e1 * f) if e0 > 0 and e1 > 0 else (e0 + e1) * f
    cell = max(cell, max(e0, e1) / 4000.0)
    if not cell > 0:
        cell = 1.0
    ny = int(min(e1 / cell, 4000.0)) + 1

    def order(A):
        ax, ay = A[:, 0].astype(np.float64), A[:, 1].astype(np.float64)
        ok = np.isfinite(ax) & np.isfinite(ay)
        bx = np.clip(np.where(ok, (ax - lo0) / cell, 0.0), 0.0, 4000.0).astype(np.int64)
        by = np.minimum(np.clip(np.where(ok, (ay - lo1) / cell, 0.0), 0.0, 4000.0).astype(np.int64), ny - 1)
        key = np.where(ok, bx * ny + np.where(bx & 1, ny - 1 - by, by), 0)
        return np.argsort(key, kind="stable")

    return order(Q), order(R)


def gaps(Q, R, perm_q, perm_r):
    """float64 [query blocks][reference blocks]: the squared box gaps; perm_q may name the rows of a range of Q only"""
    return box_gap2(block_boxes(Q, perm_q), block_boxes(R, perm_r))


def pair_bounds(g, r2max):
    """(#{gap^2 < r2max}, #{gap^2 < 1.001 r2max}) over the block pairs of the rectangle"""
    return int((g < r2max).sum()), int((g < 1.001 * r2max).sum())


def tile_bounds(Q, R, perm_q, perm_r, radii):
    """(lower, upper) for the `tiles` counter of a call: 16 tile pairs per evaluated block pair, added over its launches"""
    if len(perm_q) == 0 or len(perm_r) == 0:
        return 0, 0
    g = gaps(Q, R, perm_q, perm_r)
    lo = hi = 0
    for r2 in launch_r2max(radii):
        a, b = pair_bounds(g, r2)
        lo, hi = lo + 16 * a, hi + 16 * b
    return lo, hi


def empty_units(g, r2max):
    """(units without a block pair of gap^2 < 1.001 r2max, all units): a unit is (query block, reference share)"""
    near = g < 1.001 * r2max
    sy = shares(g.shape[1])
    per_unit = np.array([[near[q, y::sy].sum() for y in range(sy)] for q in range(g.shape[0])])
    return int((per_unit == 0).sum()), per_unit.size


@functools.lru_cache(maxsize=None)
def split_sets(n_q, n_r, n_cols):
    """stretched(n_q + n_r, D): the first n_q rows are the queries, the rest the reference"""
    c = stretched(n_q + n_r, n_cols)
    return np.ascontiguousarray(c[:n_q]), np.ascontiguousarray(c[n_q:])


# (n_q, n_r, D) -> (surviving block pairs, all block pairs) of split_sets under joint_order at the largest of
# radii_for(D, 3) -- the same for gap^2 < r2max and for gap^2 < 1.001 r2max
SPLIT_TABLE = {(300, 1500, 100): (22, 36), (1500, 1500, 65): (64, 144), (1500, 1500, 100): (64, 144), (1500, 1500, 256): (64, 144),
               (700, 2100, 100): (49, 102), (1100, 8320, 80): (243, 585)}

MIXED_RADIUS = 1e-3


@functools.lru_cache(maxsize=None)
def mixed_units_sets():
    """queries from one edge of the plane: Q the 1 100 rows of lowest column 0 of stretched(11 420, 80), R the next 8 320 of
    the remaining rows, both in row order.  At r = 1e-3 only the blocks that share a duplicate-free neighbourhood survive:
    units without a survivor sit beside units with one."""
    n_q, n_r = 1100, 8320
    c = stretched(n_q + n_r + 2000, 80)
    o = np.argsort(c[:, 0], kind="stable")
    rest = np.sort(o[n_q:])
    return np.ascontiguousarray(c[np.sort(o[:n_q])]), np.ascontiguousarray(c[rest[:n_r]])


def margin_sets():
    """widepruneref.margin_case with group A as the queries and group B as the reference, one block each
    -> (Q, R, r, (a, b, c, d)): a a row of Q; b, c, d rows of R; the box gap of the two blocks is d2(a, d), one ulp inside
    r = 3; d2(a, b) is on the radius, d2(a, c) an ulp outside"""
    c, r, (a, b, cc, d) = wp.margin_case()
    assert a % 2 == 0 and b % 2 == cc % 2 == d % 2 == 1
    return np.ascontiguousarray(c[0::2]), np.ascontiguousarray(c[1::2]), r, (a // 2, b // 2, cc // 2, d // 2)


def exact_band_pairs(n_cols, Q, R, perm_q, perm_r, radii):
    """pairs of surviving block pairs with |d2 - r^2| < eps at some radius of the call, added over the radii -- what the
    matrix-core window cannot decide (wideref.eps over Q and R together: one origin, one scale), with d2 in float64"""
    import wideref
    g = gaps(Q, R, perm_q, perm_r)
    near = g < 1.001 * max(launch_r2max(radii))
    U = np.concatenate([Q, R])
    q64, r64 = Q[perm_q].astype(np.float64), R[perm_r].astype(np.float64)
    total = 0
    for r in radii:
        r2 = float(F32(r) * F32(r))
        e = wideref.eps(n_cols, U, r2)
        for qb in range(g.shape[0]):
            rows = np.flatnonzero(near[qb])
            if len(rows) == 0:
                continue
            ref = np.concatenate([r64[BLOCK * b:BLOCK * (b + 1)] for b in rows])
            qq = q64[BLOCK * qb:BLOCK * (qb + 1)]
            d2 = (qq * qq).sum(1)[:, None] + (ref * ref).sum(1)[None, :] - 2.0 * qq @ ref.T
            total += int((np.abs(d2 - r2) < e).sum())
    return total, int(near.sum())
