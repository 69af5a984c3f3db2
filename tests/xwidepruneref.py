"""Cases and counter bounds of the pruned sweeps' tests at 257..1024 columns: tests/test_xwide_pruned_cases.py
checks their premises on the CPU with a numpy cell order, tests/test_gpu_xwide_pruned.py and tests/test_gpu_xwide_nn_pruned.py
run them on the device and take the order from the device (density.xwide_pruned_order).

Data that prunes at these widths.  widepruneref.stretched (columns 0 / 1 x 4) does not: the intra-blob distance grows like
sqrt(D) and at 1024 columns the radius exceeds the blobs' gap in the plane.  Here columns 0 / 1 are multiplied by 8 and the
radii follow the intra-blob distance of THAT layout.

The bounds are widepruneref's (populations) and widennpruneref's construction (neighbours) with the figures of these widths:
the float d2 of the device differs from float64 by at most (D + 1) 2^-24 = 6.1e-5 at 1024 columns, so the neighbour rule's
lower factor is 1 - 7e-5 here -- a constant of this module, not the 256-column one."""
import functools

import numpy as np

import wideref
import widepruneref as pr
import widennpruneref as nnref
import xwideref

F32 = np.float32
BLOCK = pr.BLOCK
STRETCH = 8
F_LO, F_HI = 1.0 - 7.0e-5, 1.001
FLT_MAX = np.finfo(np.float32).max
COLS = (257, 258, 261, 267, 272, 401, 512, 1024)   # NM mod 4 = 1, 1, 2, 3, 0; beyond 400: the chunked direct kernel; the ends
TABLE_COLS = (257, 512, 1024)

# rows -> (surviving block pairs, all block pairs) of the population sweep at the largest radius, the same at 257, 512 and
# 1024 columns and for gap^2 < r2max and gap^2 < 1.001 r2max, under the numpy cell order
POP_TABLE = {700: (20, 36), 1500: (64, 144), 2100: (119, 289)}
# (rows, columns) -> (evaluated block pairs, all block pairs) of the neighbour sweep with the free energies of the
# populations at the base radius: lower == upper
NN_TABLE = {(700, 257): (29, 36), (700, 1024): (28, 36), (1500, 257): (82, 144), (1500, 1024): (82, 144),
            (2100, 257): (140, 289), (2100, 1024): (151, 289)}
BAND_SHARE = 0.08   # the exact-path bound of the stretched 1 500-row case, of 1024 x its lower tile pairs, at most


def stretched(n_rows, n_cols, seed=7):
    """wideref.blobs with columns 0 and 1 multiplied by 8: the blobs lie 8 apart, 0.64 wide in the plane of the order"""
    c = wideref.blobs(n_rows, n_cols, seed=seed).copy()
    c[:, 0] *= F32(STRETCH)
    c[:, 1] *= F32(STRETCH)
    return np.ascontiguousarray(c)


def base_radius(n_cols):
    return float(np.sqrt(2 * 0.08 * 0.08 * (n_cols - 2) + 2 * 0.64 * 0.64))


def radii_for(n_cols):
    """three radii around the intra-blob distance of the stretched blobs, not sorted"""
    base = base_radius(n_cols)
    return [base * f for f in (1.0, 0.9, 1.08)]


def mfmas_per_tile_pair(n_cols):
    return (2 + 3 * n_cols + 15) // 16


# ---- the neighbour sweep's bounds: widennpruneref.block_sets with the factors of these widths ------------------------
def block_sets(c, fe, perm, qb, boxes=None, ranges=None):
    """(seed, S1_lo, S1_hi, lower, upper) of query block qb: boolean masks over the reference blocks"""
    nb = pr.n_blocks(len(perm))
    boxes = pr.block_boxes(c, perm) if boxes is None else boxes
    ranges = nnref.fe_ranges(fe, perm) if ranges is None else ranges
    gap = pr.box_gap2(boxes[qb:qb + 1], boxes)[0]
    nn_min, hd_min = nnref._block_minima(c, fe, perm, qb)
    seed = np.zeros(nb, dtype=bool)
    seed[nnref.seed_blocks(qb, nb)] = True
    b_nn = nnref._bound(nn_min, seed)
    with np.errstate(invalid="ignore"):
        s1_lo = seed | (gap < F_LO * b_nn)
        s1_hi = seed | (gap < F_HI * b_nn)
        fe_ok = ranges[:, 0] < ranges[qb, 1]
        lower = s1_lo | ((gap < F_LO * nnref._bound(hd_min, s1_hi)) & fe_ok)
        upper = s1_hi | ((gap < F_HI * nnref._bound(hd_min, s1_lo)) & fe_ok)
    return seed, s1_lo, s1_hi, lower, upper


_COUNTS = {}


def block_counts(c, fe, perm):
    """int64 [blocks][4]: (|lower|, |upper|, |S1_lo|, |S1_hi|) of every query block; computed once per (data, order)"""
    perm = np.ascontiguousarray(perm, dtype=np.int64)
    key = (c.shape, hash(c.tobytes()), hash(np.ascontiguousarray(fe, dtype=np.float32).tobytes()), hash(perm.tobytes()))
    if key not in _COUNTS:
        boxes, ranges = pr.block_boxes(c, perm), nnref.fe_ranges(fe, perm)
        out = np.zeros((pr.n_blocks(len(c)), 4), dtype=np.int64)
        for qb in range(len(out)):
            _, s1_lo, s1_hi, lower, upper = block_sets(c, fe, perm, qb, boxes, ranges)
            out[qb] = (lower.sum(), upper.sum(), s1_lo.sum(), s1_hi.sum())
        _COUNTS[key] = out
    return _COUNTS[key]


def nn_pair_bounds(c, fe, perm, segment=0, n_segments=0):
    """(|lower|, |upper|, |S1_lo|, |S1_hi|) in block pairs over the query blocks of a call"""
    qb = list(pr.segment_blocks(len(c), segment, n_segments))
    return tuple(int(v) for v in block_counts(c, fe, perm)[qb].sum(axis=0)) if qb else (0, 0, 0, 0)


# ---- the cases, each computed once ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pop_case(n_rows, n_cols, extra=()):
    """(coords, radii, populations): the stretched blobs at radii_for(D) + extra"""
    from oracle.oracle import Oracle
    c = stretched(n_rows, n_cols)
    radii = tuple(radii_for(n_cols)) + tuple(extra)
    return c, radii, Oracle().populations(c, list(radii))


@functools.lru_cache(maxsize=None)
def fe_case(n_rows, n_cols):
    """(coords, free energies of the populations at the base radius)"""
    from oracle.oracle import Oracle
    o = Oracle()
    c = stretched(n_rows, n_cols)
    return c, o.free_energies(o.populations(c, [base_radius(n_cols)])[0])


@functools.lru_cache(maxsize=None)
def nn_case(n_rows, n_cols):
    """(coords, those free energies, neighbours)"""
    from oracle.oracle import Oracle
    c, fe = fe_case(n_rows, n_cols)
    return c, fe, Oracle().nearest_neighbors(c, fe)


@functools.lru_cache(maxsize=None)
def stretched_band_bound(n_cols, n_rows=1500):
    """the cap on the pairs a correct population sweep of the stretched case can send to the exact path, by xwideref.band
    and the counting rule of xwideref.band_case over the three radii: ordered pairs i != j with
    |S d2 - t| <= 2 (e0 + kappa t) + margin at some radius, plus the pairs exactly at a radius"""
    c = stretched(n_rows, n_cols)
    d2 = xwideref.pair_d2(c)
    off = ~np.eye(len(c), dtype=bool)
    s, e0, kappa = xwideref.band(n_cols, c)
    near = np.zeros_like(off)
    at = 0
    for r in radii_for(n_cols):
        r2 = float(F32(r) * F32(r))
        t = s * r2
        near |= np.abs(s * d2 - t) <= 2.0 * (e0 + kappa * t) + xwideref.window_margin(t, e0)
        at += int(((d2 == r2) & off).sum())
    return int((near & off).sum()) + at
