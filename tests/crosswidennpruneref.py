"""Cases and counter bounds of the pruned wide cross neighbour sweep's tests (65..256 columns, queries against a reference,
DESIGN.md 4.26): tests/test_cross_wide_nn_pruned_cases.py checks the premises on the CPU with the numpy joint-grid order
of crosswidepruneref, tests/test_gpu_cross_wide_nn_pruned.py runs the cases on the device and takes both orders from the
device (density.wide_against_pruned_order).  Importing this module needs neither a GPU nor torch.

The pruning check is widennpruneref's with the seed set replaced.  Per query block qb (128 positions of the query order)
the sweep meets three disjoint sets of reference blocks (128 positions of the reference's order):
  seed    ONE block: the reference block whose box centre is nearest to the query block's box centre in the (col 0, col 1)
          plane, the lowest block on a tie,
  ring 1  the other blocks with box gap^2 < far2_nn[qb] = 1.0001 max(B_nn, FLT_MIN), B_nn the largest nn_d2 of the block's
          rows after the seed (finite: the seed block has a row and nothing is excluded),
  ring 2  the blocks of neither with gap^2 < far2_hd[qb] = 1.0001 max(B_hd, FLT_MIN) and fe_min[rb] < fe_max[qb], B_hd the
          largest hd_d2 of the block's rows after ring 1 (+inf where a row has none); no ring 2 without free energies.
Everything is formed in float64 from the two orders, with widennpruneref's F_LO = 1 - 2e-5 and F_HI = 1.001:
  S1_lo = seed + {G < F_LO B_nn(seed)},  S1_hi = seed + {G < F_HI B_nn(seed)}
  lower = S1_lo + {G < F_LO B_hd(S1_hi), fe_min < fe_max},  upper = S1_hi + {G < F_HI B_hd(S1_lo), fe_min < fe_max}
and the `tiles` counter of a call lies in [16 |lower|, 16 |upper|], its `mfmas` counter is tiles x mfmas_per_tile_pair(D).

The seed is formed in float64 here and in float32 on the device.  Each case carries the PREMISE that the choice is
unambiguous: per query block the least and the second-least squared centre distance differ by more than 1e-5 relative, or
the two blocks tie exactly (equal centre distance in float64 AND in the device's float32 arithmetic: the index rule
decides); seed_premise asserts it, on the CPU for the numpy order and on the GPU for the device's."""
import functools

import numpy as np

import crosswidepruneref as cp
import widennpruneref as wn
import widepruneref as pr
from widennpruneref import F_HI, F_LO, MARGIN_FAR2, mfmas_per_tile_pair

F32 = np.float32
BLOCK = pr.BLOCK
FLT_MIN = float(np.finfo(np.float32).tiny)   # the floor of wide_nn_far2


def _centre_d2(boxes_q, boxes_r, dtype):
    """[q][r] squared centre distances in the arithmetic of wide_cross_seed_key at the given precision: centres
    0.5 * (lo + hi), two differences, their squares, one sum"""
    q, r = boxes_q.astype(dtype), boxes_r.astype(dtype)
    half = dtype(0.5)
    cq0, cq1 = half * (q[:, 0] + q[:, 1]), half * (q[:, 2] + q[:, 3])
    cr0, cr1 = half * (r[:, 0] + r[:, 1]), half * (r[:, 2] + r[:, 3])
    dx, dy = cq0[:, None] - cr0[None, :], cq1[:, None] - cr1[None, :]
    return dx * dx + dy * dy


def seed_blocks(boxes_q, boxes_r, dtype=np.float64):
    """int64 [query blocks]: the seed of every query block -- argmin of the squared centre distance, the lowest block on a
    tie (every block of an order of n rows has a live row: ceil(n / 128) blocks)"""
    return np.argmin(_centre_d2(boxes_q, boxes_r, dtype), axis=1).astype(np.int64)


def seed_premise(boxes_q, boxes_r):
    """asserts that the seed of every query block is unambiguous (module docstring) -> the seeds"""
    c64, c32 = _centre_d2(boxes_q, boxes_r, np.float64), _centre_d2(boxes_q, boxes_r, np.float32)
    seeds = np.argmin(c64, axis=1).astype(np.int64)
    assert (np.argmin(c32, axis=1) == seeds).all(), "the float32 rule picks another block"
    if c64.shape[1] > 1:
        for qb, s in enumerate(seeds):
            rest = np.delete(np.arange(c64.shape[1]), s)
            k = rest[np.argmin(c64[qb, rest])]
            best, second = c64[qb, s], c64[qb, k]
            tie = best == second and c32[qb, s] == c32[qb, k]
            assert tie or second - best > 1e-5 * second, (qb, int(s), int(k), best, second)
    return seeds


def _block_minima(Q, R, fe_q, fe_r, perm_q, perm_r, qb):
    """float64 [rows of query block qb][reference blocks]: the least d2 from each row of the block to the rows of every
    reference block, and the same over the rows of lower free energy (IEEE comparison; None without free energies)"""
    perm_q, perm_r = np.asarray(perm_q, dtype=np.int64), np.asarray(perm_r, dtype=np.int64)
    n_r, nb = len(perm_r), pr.n_blocks(len(perm_r))
    x = R[perm_r].astype(np.float64)
    q = Q[perm_q[BLOCK * qb:BLOCK * (qb + 1)]].astype(np.float64)
    gq, gx = (q * q).sum(axis=1), (x * x).sum(axis=1)
    d2 = np.maximum(gq[:, None] + gx[None, :] - 2.0 * (q @ x.T), 0.0)
    # (the Gram form loses digits where d2 is tiny against the norms: the pairs that matter are re-formed directly)
    near = d2 < 1e-6 * (gq[:, None] + gx[None, :])
    for i, j in zip(*np.nonzero(near)):
        d2[i, j] = ((q[i] - x[j]) ** 2).sum()
    pad = nb * BLOCK - n_r

    def per_block(m):
        if pad:
            m = np.concatenate([m, np.full((len(q), pad), np.inf)], axis=1)
        return m.reshape(len(q), nb, BLOCK).min(axis=2)

    if fe_q is None:
        return per_block(d2), None
    fq = np.asarray(fe_q, dtype=np.float32)[perm_q[BLOCK * qb:BLOCK * (qb + 1)]]
    fr = np.asarray(fe_r, dtype=np.float32)[perm_r]
    with np.errstate(invalid="ignore"):
        lower = fr[None, :] < fq[:, None]
    return per_block(d2), per_block(np.where(lower, d2, np.inf))


def _bound(minima, blocks):
    """the largest, over the rows, of the least entry inside the given blocks (a boolean mask), not below the floor; +inf
    if a row has none"""
    if not blocks.any():
        return np.inf
    return max(float(minima[:, blocks].min(axis=1).max()), FLT_MIN)


def fe_ends(fe_q, fe_r, perm_q, perm_r):
    """(float64 [reference blocks] the least free energy, float64 [query blocks] the largest)"""
    fq = np.asarray(fe_q, dtype=np.float32)[np.asarray(perm_q, dtype=np.int64)].astype(np.float64)
    fr = np.asarray(fe_r, dtype=np.float32)[np.asarray(perm_r, dtype=np.int64)].astype(np.float64)
    return (np.array([fr[BLOCK * b:BLOCK * (b + 1)].min() for b in range(pr.n_blocks(len(fr)))]),
            np.array([fq[BLOCK * b:BLOCK * (b + 1)].max() for b in range(pr.n_blocks(len(fq)))]))


def block_sets(Q, R, fe_q, fe_r, perm_q, perm_r, qb, gap=None, seeds=None, ends=None):
    """(seed mask, S1_lo, S1_hi, lower, upper, B_nn, B_hd over S1_hi) of query block qb: boolean masks over the reference
    blocks; fe_q None: nn only, lower = S1_lo and upper = S1_hi"""
    if gap is None:
        gap = cp.gaps(Q, R, perm_q, perm_r)
    if seeds is None:
        seeds = seed_blocks(pr.block_boxes(Q, perm_q), pr.block_boxes(R, perm_r))
    nn_min, hd_min = _block_minima(Q, R, fe_q, fe_r, perm_q, perm_r, qb)
    seed = np.zeros(gap.shape[1], dtype=bool)
    seed[seeds[qb]] = True
    b_nn = _bound(nn_min, seed)
    g = gap[qb]
    s1_lo, s1_hi = seed | (g < F_LO * b_nn), seed | (g < F_HI * b_nn)
    if fe_q is None:
        return seed, s1_lo, s1_hi, s1_lo, s1_hi, b_nn, np.inf
    if ends is None:
        ends = fe_ends(fe_q, fe_r, perm_q, perm_r)
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
        gap = cp.gaps(Q, R, perm_q, perm_r)
        seeds = seed_premise(pr.block_boxes(Q, perm_q), pr.block_boxes(R, perm_r))
        ends = None if fe_q is None else fe_ends(fe_q, fe_r, perm_q, perm_r)
        counts, bounds = np.zeros((gap.shape[0], 4), dtype=np.int64), np.zeros((gap.shape[0], 2))
        for qb in range(gap.shape[0]):
            _, s1_lo, s1_hi, lower, upper, b_nn, b_hd = block_sets(Q, R, fe_q, fe_r, perm_q, perm_r, qb, gap, seeds, ends)
            counts[qb] = (lower.sum(), upper.sum(), s1_lo.sum(), s1_hi.sum())
            bounds[qb] = (b_nn, b_hd)
        _COUNTS[key] = (counts, bounds)
    return _COUNTS[key]


def pair_bounds(Q, R, fe_q, fe_r, perm_q, perm_r):
    """(|lower|, |upper|, |S1_lo|, |S1_hi|) in block pairs over the query blocks of a call"""
    if len(perm_q) == 0 or len(perm_r) == 0:
        return 0, 0, 0, 0
    return tuple(int(v) for v in block_counts(Q, R, fe_q, fe_r, perm_q, perm_r)[0].sum(axis=0))


def tile_bounds(Q, R, fe_q, fe_r, perm_q, perm_r):
    """(lower, upper) for the `tiles` counter of a call: 16 tile pairs per evaluated block pair"""
    lo, hi, _, _ = pair_bounds(Q, R, fe_q, fe_r, perm_q, perm_r)
    return 16 * lo, 16 * hi


def std_radius(n_cols):
    return pr.radii_for(n_cols, 3)[0]


def pops_pair(Q, R, radius):
    """(populations of the queries in R, populations of the reference in itself -- each row counts itself) at one radius,
    in float64 (the tests need free energies of that kind, not populations bit for bit)"""
    r2 = float(F32(radius) * F32(radius))
    r64, q64 = R.astype(np.float64), Q.astype(np.float64)
    gr, gq = (r64 * r64).sum(axis=1), (q64 * q64).sum(axis=1)
    pops_r = np.maximum(((gr[:, None] + gr[None, :] - 2.0 * r64 @ r64.T) < r2).sum(axis=1), 1)
    pops_q = ((gq[:, None] + gr[None, :] - 2.0 * q64 @ r64.T) < r2).sum(axis=1)
    return pops_q.astype(np.int64), pops_r.astype(np.int64)


@functools.lru_cache(maxsize=None)
def split_case(n_q, n_r, n_cols):
    """(Q, R, fe_q, fe_r): crosswidepruneref.split_sets with the free energies of the populations at std_radius -- the
    reference's own, the queries' against the reference, both over the reference's largest population as
    calculate_free_energies_against scales them; +inf for a query without a reference inside the radius"""
    Q, R = cp.split_sets(n_q, n_r, n_cols)
    pops_q, pops_r = pops_pair(Q, R, std_radius(n_cols))
    top = float(pops_r.max())
    with np.errstate(divide="ignore"):
        fe_r = (-np.log(pops_r / top)).astype(np.float32)
        fe_q = np.where(pops_q > 0, -np.log(np.maximum(pops_q, 1) / top), np.inf).astype(np.float32)
    return Q, R, np.ascontiguousarray(fe_q), np.ascontiguousarray(fe_r)


# (n_q, n_r, D) -> (evaluated block pairs, all block pairs) of split_case under joint_order: lower == upper at every shape
SPLIT_TABLE = {(300, 1500, 100): (25, 36), (1500, 1500, 65): (71, 144), (1500, 1500, 256): (71, 144), (700, 2100, 100): (59, 102),
               (1100, 8320, 80): (243, 585)}


@functools.lru_cache(maxsize=None)
def cross_block_tie_sets(n_cols=100):
    """-> (Q, R, fe_q, fe_r, (a_q, p, q)): widennpruneref.cross_block_tie_case over two sets.  R is its 384 rows with row a
    moved far off in column 2, so that the reference still has its three blocks and nothing lies at a's place; Q is the
    middle group, a among it at query row a_q.  d2(a, p) = d2(a, q) = 9 exactly, every other reference is further than 9
    from a, p (a HIGH row) lies in the block the reference's order puts first and q (a LOW row) in the block it puts
    last, fe[p] = fe[q] < fe[a]: nn and nn_hd of a are row q.  A merge on positions would answer p."""
    c, fe, (a, p, q) = wn.cross_block_tie_case(n_cols)
    middle = np.arange(1, len(c), 3)
    R = c.copy()
    R[a, 2] += F32(50.0)
    a_q = int(np.flatnonzero(middle == a)[0])
    return np.ascontiguousarray(c[middle]), np.ascontiguousarray(R), np.ascontiguousarray(fe[middle]), fe.copy(), (a_q, p, q)


@functools.lru_cache(maxsize=None)
def margin_sets(which, n_cols=80):
    """-> (Q, R, fe_q, fe_r, a_q, gap2): widennpruneref.margin_case over two sets.  Q is its group A, one query block, with
    row a at (0, 0) at query row a_q.  R is three groups the reference's order puts into one block each: a copy of group A
    in which a's row is replaced by a second copy of a2 (every query but a has an exact copy there, a has a2 at d2 = 9
    exactly: the bound of the query block after its seed launch is 9, far2_nn = MARGIN_FAR2), then M and B as they are.
    The seed of the query block is the copy of A (the centres nearly coincide; M and B lie 3 and more away); M is in ring 1
    (gap^2 = 1.44); the gap of the query block and B is fl(9 + fl(dy^2)), one ulp inside MARGIN_FAR2 (which = -1: ring 1),
    on it (0: not met) or one ulp outside (+1: not met).  Constant free energies: ring 2 is empty."""
    c, _, (a, a2), target = wn.margin_case(which, n_cols)
    n = len(c)
    A, M, B = (np.sort(np.concatenate([np.arange(g, n, 6), np.arange(g + 1, n, 6)])) for g in (0, 2, 4))
    Q = c[A].copy()
    a_q = int(np.flatnonzero(A == a)[0])
    RA = c[A].copy()
    RA[a_q] = c[a2]
    groups = np.concatenate([RA, c[M], c[B]])
    R = np.empty_like(groups)
    R[np.argsort(np.arange(n) % 3, kind="stable")] = groups   # (interleaved -- rows 3k, 3k + 1, 3k + 2 --: the order has to sort them)
    return (np.ascontiguousarray(Q), np.ascontiguousarray(R), np.zeros(len(Q), dtype=np.float32),
            np.zeros(len(R), dtype=np.float32), a_q, float(target))


def shifted_gradient(Q, R):
    """(fe_q, fe_r) = (column 0 of Q - 2, column 0 of R): the blobs of the stretched sets lie 4 apart along column 0 and are
    0.32 wide, so every reference of a query's own blob lies HIGHER and every reference of the blobs to its left lower --
    after ring 1 a query has no lower reference, its block's B_hd is +inf, and ring 2 meets every block that holds a lower
    row; the queries of the leftmost blob have no lower reference at all"""
    return np.ascontiguousarray(Q[:, 0] - F32(2.0)), np.ascontiguousarray(R[:, 0])


def far_sets(n_q=300, n_r=1500, n_cols=100):
    """split_case with the queries moved 100 along column 0: far from the whole reference, every box gap is about 10^4"""
    Q, R, fe_q, fe_r = split_case(n_q, n_r, n_cols)
    Q = Q.copy()
    Q[:, 0] += F32(100.0)
    return np.ascontiguousarray(Q), R, fe_q, fe_r
