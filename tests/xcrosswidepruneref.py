"""Cases and counter bounds of the pruned cross sweeps' tests at 257..1024 columns (queries against a reference, DESIGN.md
4.34): tests/test_cross_xwide_pruned_cases.py checks their premises on the CPU with the numpy joint-grid order of
crosswidepruneref, tests/test_gpu_cross_xwide_pruned.py and tests/test_gpu_cross_xwide_nn_pruned.py run them on the device
and take both orders from the device (density.xwide_against_pruned_order).  Importing this module needs neither a GPU nor
torch.

Everything is built from what exists: the data of xwidepruneref (columns 0 / 1 x 8, its radii), the joint order, the gaps
and the population bounds of crosswidepruneref, and crosswidennpruneref's construction of the neighbour bounds with the
constants of these widths in place of 1 - 2e-5 and FLT_MIN: F_LO = 1 - 7e-5 (the float d2 of the device differs from
float64 by at most (D + 2) 2^-24 = 6.1e-5 at 1024 columns), F_HI = 1.001 and the floor 2^-122 of wide_nn_far2 beyond 256
columns."""
import functools

import numpy as np

import crosswidennpruneref as cn
import crosswidepruneref as cp
import widepruneref as pr
import xwidepruneref as xp
import xwideref
from crosswidepruneref import gaps, joint_order, query_blocks, tile_bounds  # noqa: F401  (the population sweep's bounds)
from xwidepruneref import BAND_SHARE, COLS, F_HI, F_LO, base_radius, mfmas_per_tile_pair, radii_for, stretched  # noqa: F401

F32 = np.float32
BLOCK = pr.BLOCK
FLOOR = 2.0 ** -122          # wide_nn_floor / wide_pop_floor beyond 256 columns
FLT_MAX = float(np.finfo(np.float32).max)
n_blocks = pr.n_blocks

# (n_q, n_r) -> (surviving block pairs, all block pairs) of split_sets under joint_order at the largest of radii_for(D) --
# the same for gap^2 < r2max and for gap^2 < 1.001 r2max, at each of the columns checked
POP_TABLE = {(300, 1500): (22, 36), (1500, 1500): (64, 144), (700, 2100): (49, 102), (1100, 8320): (243, 585)}
POP_COLS = {(300, 1500): (257, 1024), (1500, 1500): (257, 512, 1024), (700, 2100): (257, 1024), (1100, 8320): (257,)}
# (n_q, n_r, D) -> (block pairs met with the free energies of split_case, block pairs met nn only): lower == upper
NN_TABLE = {(300, 1500, 257): (22, 22), (300, 1500, 1024): (25, 25), (1500, 1500, 257): (85, 64), (1500, 1500, 512): (78, 64),
            (1500, 1500, 1024): (88, 64), (700, 2100, 257): (49, 49), (700, 2100, 1024): (59, 49), (1100, 8320, 257): (307, 243)}
# D -> the pairs of the 1 500 x 1 500 split inside xwideref.band at some radius of radii_for(D), in float64
BAND_PAIRS = {257: 29011, 512: 38622, 1024: 58646}
NN_EXACT_SHARE = 0.05   # the neighbour sweep's exact-path cap, of 1024 x tiles: test_gpu_xwide_nn_pruned.py's


@functools.lru_cache(maxsize=None)
def split_sets(n_q, n_r, n_cols):
    """xwidepruneref.stretched(n_q + n_r, D): the first n_q rows are the queries, the rest the reference"""
    c = stretched(n_q + n_r, n_cols)
    return np.ascontiguousarray(c[:n_q]), np.ascontiguousarray(c[n_q:])


@functools.lru_cache(maxsize=None)
def split_case(n_q, n_r, n_cols):
    """(Q, R, fe_q, fe_r): split_sets with the free energies of the populations at base_radius(D), scaled as
    crosswidennpruneref.split_case scales them (over the reference's largest population; +inf for a query with no reference
    inside the radius)"""
    Q, R = split_sets(n_q, n_r, n_cols)
    pops_q, pops_r = cn.pops_pair(Q, R, base_radius(n_cols))
    top = float(pops_r.max())
    with np.errstate(divide="ignore"):
        fe_r = (-np.log(pops_r / top)).astype(np.float32)
        fe_q = np.where(pops_q > 0, -np.log(np.maximum(pops_q, 1) / top), np.inf).astype(np.float32)
    return Q, R, np.ascontiguousarray(fe_q), np.ascontiguousarray(fe_r)


# ---- the neighbour sweep's bounds: crosswidennpruneref.block_sets with the constants of these widths -----------------
def _bound(minima, blocks):
    """the largest, over the rows, of the least entry inside the given blocks (a boolean mask), not below the floor of
    these widths; +inf if a row has none"""
    if not blocks.any():
        return np.inf
    return max(float(minima[:, blocks].min(axis=1).max()), FLOOR)


def block_sets(Q, R, fe_q, fe_r, perm_q, perm_r, qb, gap=None, seeds=None, ends=None):
    """(seed mask, S1_lo, S1_hi, lower, upper, B_nn, B_hd over S1_hi) of query block qb: boolean masks over the reference
    blocks; fe_q None: nn only, lower = S1_lo and upper = S1_hi"""
    if gap is None:
        gap = gaps(Q, R, perm_q, perm_r)
    if seeds is None:
        seeds = cn.seed_blocks(pr.block_boxes(Q, perm_q), pr.block_boxes(R, perm_r))
    nn_min, hd_min = cn._block_minima(Q, R, fe_q, fe_r, perm_q, perm_r, qb)
    seed = np.zeros(gap.shape[1], dtype=bool)
    seed[seeds[qb]] = True
    b_nn = _bound(nn_min, seed)
    g = gap[qb]
    s1_lo, s1_hi = seed | (g < F_LO * b_nn), seed | (g < F_HI * b_nn)
    if fe_q is None:
        return seed, s1_lo, s1_hi, s1_lo, s1_hi, b_nn, np.inf
    if ends is None:
        ends = cn.fe_ends(fe_q, fe_r, perm_q, perm_r)
    with np.errstate(invalid="ignore"):
        fe_ok = ends[0] < ends[1][qb]
        b_hd = _bound(hd_min, s1_hi)
        lower = s1_lo | ((g < F_LO * b_hd) & fe_ok)
        upper = s1_hi | ((g < F_HI * _bound(hd_min, s1_lo)) & fe_ok)
    return seed, s1_lo, s1_hi, lower, upper, b_nn, b_hd


_COUNTS = {}


def block_counts(Q, R, fe_q, fe_r, perm_q, perm_r):
    """(int64 [query blocks][4] = (|lower|, |upper|, |S1_lo|, |S1_hi|), float64 [query blocks][2] = (B_nn, B_hd)); once per
    (data, orders).  Asserts the seed premise on these orders."""
    perm_q, perm_r = np.ascontiguousarray(perm_q, dtype=np.int64), np.ascontiguousarray(perm_r, dtype=np.int64)
    fb = lambda f: b"" if f is None else np.ascontiguousarray(f, dtype=np.float32).tobytes()
    key = (Q.shape, R.shape, hash(Q.tobytes()), hash(R.tobytes()), hash(fb(fe_q)), hash(fb(fe_r)), hash(perm_q.tobytes()),
           hash(perm_r.tobytes()))
    if key not in _COUNTS:
        gap = gaps(Q, R, perm_q, perm_r)
        seeds = cn.seed_premise(pr.block_boxes(Q, perm_q), pr.block_boxes(R, perm_r))
        ends = None if fe_q is None else cn.fe_ends(fe_q, fe_r, perm_q, perm_r)
        counts, bounds = np.zeros((gap.shape[0], 4), dtype=np.int64), np.zeros((gap.shape[0], 2))
        for qb in range(gap.shape[0]):
            _, s1_lo, s1_hi, lower, upper, b_nn, b_hd = block_sets(Q, R, fe_q, fe_r, perm_q, perm_r, qb, gap, seeds, ends)
            counts[qb] = (lower.sum(), upper.sum(), s1_lo.sum(), s1_hi.sum())
            bounds[qb] = (b_nn, b_hd)
        _COUNTS[key] = (counts, bounds)
    return _COUNTS[key]


def nn_pair_bounds(Q, R, fe_q, fe_r, perm_q, perm_r):
    """(|lower|, |upper|, |S1_lo|, |S1_hi|) in block pairs over the query blocks of a call"""
    if len(perm_q) == 0 or len(perm_r) == 0:
        return 0, 0, 0, 0
    return tuple(int(v) for v in block_counts(Q, R, fe_q, fe_r, perm_q, perm_r)[0].sum(axis=0))


def nn_tile_bounds(Q, R, fe_q, fe_r, perm_q, perm_r):
    """(lower, upper) for the `tiles` counter of a neighbour call: 16 tile pairs per evaluated block pair"""
    lo, hi, _, _ = nn_pair_bounds(Q, R, fe_q, fe_r, perm_q, perm_r)
    return 16 * lo, 16 * hi


# ---- the exact-path cap of the population sweep ---------------------------------------------------------------------
def cross_d2(Q, R):
    """float64 [n_q][n_r] squared distances"""
    q, r = Q.astype(np.float64), R.astype(np.float64)
    return np.maximum((q * q).sum(axis=1)[:, None] + (r * r).sum(axis=1)[None, :] - 2.0 * (q @ r.T), 0.0)


@functools.lru_cache(maxsize=None)
def band_pairs(n_cols, n_q=1500, n_r=1500):
    """the pairs (query, reference) of the split inside xwideref.band -- one origin and one scale over Q and R together --
    at some radius of radii_for(D): |S d2 - t| <= 2 (e0 + kappa t) + margin, plus the pairs exactly at a radius"""
    Q, R = split_sets(n_q, n_r, n_cols)
    d2 = cross_d2(Q, R)
    s, e0, kappa = xwideref.band(n_cols, np.concatenate([Q, R]))
    near = np.zeros(d2.shape, dtype=bool)
    at = 0
    for r in radii_for(n_cols):
        r2 = float(F32(r) * F32(r))
        t = s * r2
        near |= np.abs(s * d2 - t) <= 2.0 * (e0 + kappa * t) + xwideref.window_margin(t, e0)
        at += int((d2 == r2).sum())
    return int(near.sum()) + at


# ---- edge data -------------------------------------------------------------------------------------------------------
def margin_sets(n_cols):
    """widepruneref.margin_case at these widths, split as crosswidepruneref.margin_sets splits it: the even rows (group
    A) are the queries, the odd rows (group B) the reference, one block each -> (Q, R, r, (a, b, c, d)): a a row of Q; b, c,
    d rows of R; the box gap of the two blocks is d2(a, d), one ulp inside r = 3"""
    c, r, (a, b, cc, d) = pr.margin_case(n_cols)
    assert a % 2 == 0 and b % 2 == cc % 2 == d % 2 == 1
    return np.ascontiguousarray(c[0::2]), np.ascontiguousarray(c[1::2]), r, (a // 2, b // 2, cc // 2, d // 2)


def nn_margin_sets(which, n_cols):
    """crosswidennpruneref.margin_sets at these widths: the gap of the query block and the far block one ulp below
    (which = -1), on (0) and one ulp above (+1) far2_nn = fl(1.0001f x 9)"""
    return cn.margin_sets(which, n_cols)


def cross_block_tie_sets(n_cols=300):
    return cn.cross_block_tie_sets(n_cols)


def far_sets(n_q=300, n_r=1500, n_cols=300):
    """split_case with the queries moved 100 along column 0: far from the whole reference"""
    Q, R, fe_q, fe_r = split_case(n_q, n_r, n_cols)
    Q = Q.copy()
    Q[:, 0] += F32(100.0)
    return np.ascontiguousarray(Q), R, fe_q, fe_r


TINY_RADIUS = 1e-20   # fl32(r * r) is subnormal: below the floor of these widths


@functools.lru_cache(maxsize=None)
def duplicate_sets(n_q=300, n_r=1500, n_cols=300):
    """split_sets with every tenth query replaced by a copy of a reference row (query 10 k: row 7 k + 3 of R) -> (Q, R,
    copies): copies[q] = the reference row query q copies, -1 for the others"""
    Q, R = split_sets(n_q, n_r, n_cols)
    Q = Q.copy()
    copies = np.full(n_q, -1, dtype=np.int64)
    for k, q in enumerate(range(0, n_q, 10)):
        copies[q] = (7 * k + 3) % n_r
        Q[q] = R[copies[q]]
    return np.ascontiguousarray(Q), R, copies


@functools.lru_cache(maxsize=None)
def unpruned_sets(n_cols, n_q=500):
    """xwideref.band_case (unstretched blobs, radii at the 25 % and 5 % quantiles of its pair distances) split into its
    first n_q rows and the rest: nothing to prune -> (Q, R, radii)"""
    c, radii, _, _ = xwideref.band_case(n_cols)
    return np.ascontiguousarray(c[:n_q]), np.ascontiguousarray(c[n_q:]), list(radii)
