"""Cases of the tests of the radius graph on the matrix-core sweeps of 257..1024 columns, unpruned and pruned (DESIGN.md
4.37): tests/test_xwide_graph_cases.py checks their premises on the CPU with a numpy cell order and computes the
block-pair bounds the GPU counters are held to, tests/test_gpu_xwide_graph.py runs them on the device and takes the order
from the device (density.xwide_pruned_order).  The data are the stretched blobs of the pruned sweeps of these widths
(tests/xwidepruneref.py), the boundary groups of the wide sweeps (tests/wideref.py) and the lattice shapes of the graph
tests (tests/graphref.py) embedded in wide rows; the referees are graphref's over the probe's canonical d2 matrix.
Importing this module needs neither a GPU nor torch."""
import functools

import numpy as np

import widegraphpruneref as wgp
import widegraphref as wg
import widepruneref as pr
import wideref
import xwidepruneref as xp

F32 = np.float32
BLOCK = pr.BLOCK
COLS, TABLE_COLS = xp.COLS, xp.TABLE_COLS
STRETCHED_ROWS = tuple(sorted(xp.POP_TABLE))   # 700: 6 blocks; 1 500: 12 blocks, one share; 2 100: 17 blocks, two shares
MIN_EDGE_SHAPE = (700, 257)                    # 6 blocks: 3 segments of two blocks each, 7 segments of which one is empty
SMALL_RADIUS = 1.0e-3                          # holds the duplicated rows only
SMALL_RADIUS_SHAPE = (8320, 257)               # 65 blocks in 8 shares: (query block, share) units without a survivor
BOUNDARY_SHAPE = (300, 1024)
FLAWS = ("nan cell", "inf cell", "1e20 row")
FLAGGED_COLS = (300, 401)                      # the generic direct kernel | the column-chunked one (beyond 400 columns)


def stretched_radius(n_cols):
    """-> (r, r2): the largest of xwidepruneref.radii_for(n_cols), the radius xwidepruneref.POP_TABLE was made for, and
    fl32(r * r) as the graph calls take it"""
    r = max(xp.radii_for(n_cols))
    return r, wg.square(r)


def stretched_case(n_rows, n_cols):
    """-> (coords, r, r2)"""
    r, r2 = stretched_radius(n_cols)
    return xp.stretched(n_rows, n_cols), r, r2


def blob_case(n_rows, n_cols):
    """-> (coords, r, r2): unstretched blobs at their intra-blob distance (nothing to prune at these widths)"""
    return wg.blob_case(n_rows, n_cols)


def boundary_case():
    """-> (coords, r, r2, groups): wideref.boundary_case at 1024 columns: per group (a, b, c, d) the pair (a, b) ON the
    radius (d2 = 9 = r2), (a, c) one ulp outside, (a, d) one ulp inside, in every summation order"""
    c, r, groups = wideref.boundary_case(*BOUNDARY_SHAPE)
    return c, r, wg.square(r), groups


def min_edge_case():
    """-> (coords, r, r2, duplicates): the stretched blobs of MIN_EDGE_SHAPE with duplicated rows (partners tied at d2 = 0)"""
    r, r2 = stretched_radius(MIN_EDGE_SHAPE[1])
    c, dups = wgp.with_duplicates(xp.stretched(*MIN_EDGE_SHAPE))
    return c, r, r2, dups


def small_radius_case():
    """-> (coords, r, r2, duplicates): stretched blobs with duplicated rows at a radius that holds the duplicates only"""
    c, dups = wgp.with_duplicates(xp.stretched(*SMALL_RADIUS_SHAPE))
    return c, SMALL_RADIUS, wg.square(SMALL_RADIUS), dups


def flawed(c, flaw):
    """one of FLAWS put into a copy of c (rows 131, 40, 200: c needs 201 rows and 8 columns)"""
    c = c.copy()
    if flaw == "nan cell":
        c[131, 7] = np.nan
    elif flaw == "inf cell":
        c[40, c.shape[1] - 1] = np.inf
    else:
        assert flaw == "1e20 row"
        c[200, 0] = F32(1e20)
    return c


def embedded(c, n_cols):
    return wg.embedded(c, n_cols)


def tile_bounds_r2(c, perm, r2, segment=0, n_segments=0):
    """(lower, upper) of the `tiles` counter of a pruned graph call given the square r2: 16 #{gap^2 < r2} and
    16 #{gap^2 < 1.001 r2} over the block pairs of the call's query blocks, the boxes formed in float64 from the order.
    The device's rule is gap^2 < 1.0001f max(r2, 2^-122) with a few roundings of 2^-24: between the two for every r2 of the
    cases (all far above the floor)."""
    assert not (0.0 < float(r2) < 1.0e-30), "the bounds do not model the floor of these widths"
    return wgp.tile_bounds_r2(c, perm, r2, segment, n_segments)


def all_tiles(n_rows):
    """the tile pairs an unpruned whole call evaluates: 16 per block pair"""
    nb = pr.n_blocks(n_rows)
    return 16 * nb * nb


def block_rows(n_rows, n_segments):
    """the formula of DESIGN.md 4.27 for the rows of a neighbour block: the larger of the largest segment in positions and
    the largest row block, plus the 32 header entries"""
    if n_rows == 0 or n_segments == 0:
        return 0
    row_block = n_rows - (n_segments - 1) * (n_rows // n_segments)
    most = -(-pr.n_blocks(n_rows) // n_segments)
    return max(row_block, most * BLOCK) + 32


# ---- the neighbour blocks of a sharded run (tests/test_gpu_xwide_blocks.py) ------------------------------------------------
BLOCK_COLS = (257, 401, 1024)
BLOCK_ROWS = (1, 2, 129, 300, 700, 1500)
BLOCK_SEGMENTS = (2, 3, 5, 8)
TAMPERED_WORDS = (0, 1, 3, 5, 6)
NO_ORDER_MARK = 0x6E6E5700 | 2    # the header word 0 of a pack in a workspace that holds no signed order of the shape
DUPLICATE_SEGMENTS = 2            # duplicate_tie_case: the duplicates close block 0 (segment 0) and open block 1 (segment 1)
FLAW = (131, 7)


@functools.lru_cache(maxsize=None)
def duplicate_tie_case(n_cols=300):
    """-> (coords, fe, (a, p, m)): widesessionref.duplicate_tie_case at these widths -- widennpruneref.cross_block_tie_case
    with row m of the middle group made an exact copy of p (free energy included) and q moved out of the tie.  p, the
    lower row, is the last position of block 0 and m the first of block 1, where a lies too; d2(a, p) = d2(a, m) = 9 in
    every summation order, and fe[p] = fe[m] < fe[a]: nn and hd of a are p, the lower row of two duplicates that sit in
    blocks of different segments."""
    import widennpruneref as nnref
    c, fe, (a, p, q) = nnref.cross_block_tie_case(n_cols)
    c, fe = c.copy(), fe.copy()
    m = 376
    assert m % 3 == 1 and m != a and m > p, "a row of the middle group behind p"
    c[m], fe[m] = c[p], fe[p]
    c[q, 0] = F32(3.5)
    return np.ascontiguousarray(c), np.ascontiguousarray(fe), (a, p, m)


@functools.lru_cache(maxsize=None)
def nan_cell_case(n_cols, n_rows=300):
    """(coords with one NaN cell, fe, the oracle's neighbours): the statistics pass flags the data"""
    from oracle.oracle import Oracle
    c, fe = xp.fe_case(n_rows, n_cols)
    c = c.copy()
    c[FLAW] = np.nan
    return c, fe, Oracle().nearest_neighbors(c, fe)


@functools.lru_cache(maxsize=None)
def nan_fe_case(n_cols, n_rows=300):
    """(coords, fe with NaN among them, the oracle's neighbours): a NaN free energy flags the data of a neighbour call"""
    import fe_families
    from oracle.oracle import Oracle
    o = Oracle()
    c = xp.stretched(n_rows, n_cols)
    fe = fe_families.make("nan", c, o.populations(c, [xp.base_radius(n_cols)])[0])
    return c, fe, o.nearest_neighbors(c, fe)
