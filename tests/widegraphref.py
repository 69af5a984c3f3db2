"""Case generators of the tests of the radius graph on the wide matrix-core sweep (65..256 columns):
tests/test_wide_graph_cases.py checks their premises on the CPU, tests/test_gpu_wide_graph.py runs them on the device.
The referees are those of the existing graph tests (tests/graphref.py) over the probe's canonical d2 matrix; the data are
the wide sweeps' cases (tests/wideref.py) and the lattice shapes of graphref embedded in wide rows.  Importing this module
needs neither a GPU nor torch."""
import numpy as np

import graphref
import wideref

F32 = np.float32

COLS = (65, 84, 85, 128, 256)             # at 200 rows; 84 | 85: 16 | 17 MFMAs, the seam of the 4-MFMA LDS chunk
ROWS = (1, 2, 33, 129, 1500, 2100)        # at 100 columns; 1 500: 12 blocks, one share; 2 100: 17 blocks, two shares
SPARSE_SHAPE = (4100, 65)                 # 33 blocks, four shares
SPARSE_RADIUS = 0.669                     # around the 3e-4 quantile of the d2 of that shape: a few thousand pairs
BLOCK_ROWS = 128                          # rows of a workgroup's block (kWideBlockRows)


def blob_radius(n_cols):
    """the intra-blob distance of synth.gaussian_blobs (d2 ~ 2 sigma^2 D): the first radius of
    test_gpu_wide_mfma.radii_for"""
    return float(np.sqrt(2 * 0.08 * 0.08 * n_cols))


def square(r):
    """fl32(r * r): the squared radius the population sweeps compare with, handed to the graph calls as it is"""
    return F32(F32(r) * F32(r))


def blob_case(n_rows, n_cols):
    """-> (coords, r, r2)"""
    r = blob_radius(n_cols)
    return wideref.blobs(n_rows, n_cols), r, square(r)


def sparse_case():
    c = wideref.blobs(*SPARSE_SHAPE)
    return c, SPARSE_RADIUS, square(SPARSE_RADIUS)


def shares_of(n_rows):
    """reference shares of a launch over n_rows (wide_shares: a power of two, at most 64, every share >= 8 blocks)"""
    blocks = -(-(-(-n_rows // 32)) // 4)
    s = 1
    while 2 * s <= 64 and 2 * s * 8 <= blocks:
        s *= 2
    return s


def split_pairs(pairs, n_rows):
    """the pairs whose two ends lie in different query blocks AND in different reference shares (share of a row =
    its block modulo the shares)"""
    b = np.asarray(pairs) // BLOCK_ROWS
    s = b % shares_of(n_rows)
    return pairs[(b[:, 0] != b[:, 1]) & (s[:, 0] != s[:, 1])]


def embedded(c, n_cols):
    """a lattice shape of graphref in wide rows: its columns first, zeros behind (every d2 stays what it was)"""
    out = np.zeros((len(c), n_cols), dtype=np.float32)
    out[:, :c.shape[1]] = c
    return out


def chain_case(n, n_cols):
    """-> (coords, r2): consecutive frames 1 apart, all others >= 4; r2 = 2 joins the consecutive ones only"""
    return embedded(graphref.chain(n), n_cols), F32(2.0)


FLAGGED_ROWS = (17, 400, 401)


def with_non_finite(c):
    """the rows test_gpu_screening_wide.with_non_finite spoils: an inf, a NaN and a -inf in single cells"""
    c = c.copy()
    D = c.shape[1]
    c[17, 3 % D] = np.inf
    c[400, 0] = np.nan
    c[401, D - 1] = -np.inf
    return c


def rank_rule_witnesses(pairs, comp, rank):
    """(queries whose lightest eligible partner has a HIGHER rank than the query, ... a LOWER rank): the two branches of
    the smallest-rank rule.  By the definition: per query the partner of another component with the smallest key
    (max rank << 32 | min rank)."""
    n = len(comp)
    both = np.concatenate([pairs, pairs[:, ::-1]])
    q, p = both[:, 0], both[:, 1]
    ok = comp[q] != comp[p]
    q, p = q[ok], p[ok]
    rq, rp = rank[q].astype(np.uint64), rank[p].astype(np.uint64)
    key = (np.maximum(rq, rp) << np.uint64(32)) | np.minimum(rq, rp)
    best = np.full(n, graphref.ALL_ONES, dtype=np.uint64)
    np.minimum.at(best, q, key)
    has = best != graphref.ALL_ONES
    hi, lo = (best >> np.uint64(32)), (best & np.uint64(0xFFFFFFFF))
    own = rank.astype(np.uint64)
    higher = has & (lo == own)      # key = (partner, query): the partner ranks above the query
    lower = has & (hi == own)       # key = (query, partner)
    assert (higher ^ lower)[has].all()
    return int(higher.sum()), int(lower.sum())
