"""Cases of the tests of the PRUNED radius graph on the wide matrix-core sweep (65..256 columns):
tests/test_wide_graph_pruned_cases.py checks their premises on the CPU with a numpy cell order,
tests/test_gpu_wide_graph_pruned.py runs them on the device and takes the order from the device.  The data are the
stretched blobs of the pruned population sweep (tests/widepruneref.py) and the boundary cases of the wide sweeps; the
referees are those of the radius graph (tests/graphref.py, tests/widegraphref.py).  Importing this module needs neither
a GPU nor torch."""
import numpy as np

import widegraphref as wg
import widepruneref as ref

F32 = np.float32
BLOCK = ref.BLOCK
STRETCHED = tuple(sorted(ref.STRETCHED_TABLE))   # (700, 100), (1500, 100), (2100, 100): 17 blocks, two shares; (8320, 80): 65 blocks
MIN_EDGE_SHAPE = (700, 100)                      # 6 blocks: 3 segments of two blocks, 7 segments of which one is empty
SMALL_RADIUS = 1.0e-3                            # holds the duplicated rows only: most (query block, share) units have no survivor
# wideref.boundary_case(300, 80): the groups (a, b, c, d) whose row a lies in another block of the order than b, c and d --
# their boundary pairs are met across two blocks; the rows of the last group share a block (a, b, d) or not (c)
BOUNDARY_SHAPE = (300, 80)
BOUNDARY_SPLIT_GROUPS = (0, 1)


def stretched_radius(n_cols):
    """-> (r, r2): the radius widepruneref.STRETCHED_TABLE was made for, the largest of radii_for(n_cols, 3), and
    fl32(r * r) as the graph calls take it"""
    r = max(ref.radii_for(n_cols, 3))
    return r, wg.square(r)


def with_duplicates(c, k=24, seed=5):
    """-> (coords, [k, 2] (copy, original)): k rows overwritten with copies of k other rows (d2 = 0 between them)"""
    c = c.copy()
    rows = np.random.default_rng(seed).permutation(len(c))[:2 * k]
    copy, orig = rows[:k], rows[k:]
    c[copy] = c[orig]
    return np.ascontiguousarray(c), np.stack([copy, orig], axis=1).astype(np.int64)


def stretched_case(n_rows, n_cols):
    """-> (coords, r, r2): widepruneref.stretched at the radius of the table"""
    r, r2 = stretched_radius(n_cols)
    return ref.stretched(n_rows, n_cols), r, r2


def min_edge_case():
    """-> (coords, r, r2, duplicates): the stretched blobs of MIN_EDGE_SHAPE with duplicated rows (partners tied at d2 = 0)"""
    r, r2 = stretched_radius(MIN_EDGE_SHAPE[1])
    c, dups = with_duplicates(ref.stretched(*MIN_EDGE_SHAPE))
    return c, r, r2, dups


def small_radius_case():
    """-> (coords, r, r2, duplicates): 8 320 x 80 in 65 blocks and 8 shares at a radius that holds the duplicates only"""
    c, dups = with_duplicates(ref.stretched(8320, 80))
    return c, SMALL_RADIUS, wg.square(SMALL_RADIUS), dups


def inverse(perm):
    """row -> position"""
    inv = np.empty(len(perm), dtype=np.int64)
    inv[np.asarray(perm, dtype=np.int64)] = np.arange(len(perm))
    return inv


def pairs_against_the_order(pairs, perm):
    """the pairs (i, j), i < j, whose rows stand the other way round in the order: position of j < position of i.  The
    meeting that emits such a pair has reference POSITION < query POSITION and so reference row j > query row i: a sink
    that took i < j on rows at one decision point would emit it twice or never."""
    inv = inverse(perm)
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return p[inv[p[:, 1]] < inv[p[:, 0]]]


def blocks_of(rows, perm):
    """block of the order of every given row"""
    return (inverse(perm)[np.asarray(rows, dtype=np.int64)] // BLOCK).tolist()


def pairs_float64(c, r2, slack=1.0e-5):
    """[n, 2] int64, i < j: the pairs CLEARLY inside r2 (d2 < r2 (1 - slack) in float64) -- a CPU premise that holds in
    every summation order; not a referee"""
    x = c.astype(np.float64)
    sq = (x * x).sum(axis=1)
    d2 = sq[:, None] + sq[None, :] - 2.0 * (x @ x.T)
    ii, jj = np.nonzero(np.triu(d2 < float(r2) * (1.0 - slack), k=1))
    return np.stack([ii, jj], axis=1).astype(np.int64)


def tile_bounds_r2(c, perm, r2, segment=0, n_segments=0):
    """widepruneref.tile_bounds for a call that is given the SQUARE (a NaN or negative square counts as 0)"""
    r2 = float(r2)
    r2 = r2 if r2 > 0.0 else 0.0
    a, b = ref.pair_bounds(ref.block_boxes(c, perm), r2, ref.segment_blocks(len(c), segment, n_segments))
    return 16 * a, 16 * b
