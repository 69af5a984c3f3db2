"""Cases and counter bounds of the pruned wide neighbour sweep's tests (65..256 columns):
tests/test_wide_nn_pruned_cases.py checks the premises on the CPU with a numpy cell order, tests/test_gpu_wide_nn_pruned.py
runs the cases on the device and takes the order from the device (density.wide_pruned_order).

The pruning check is a condition on the counters, not a measurement.  The sweep meets, per query block qb of 128
positions of the order, three disjoint sets of reference blocks:
  seed    qb - 1, qb, qb + 1 (clamped to the blocks there are),
  ring 1  the other blocks with box gap^2 < far2_nn[qb] = 1.0001 B_nn, B_nn the largest nn_d2 of the block's rows after the seed,
  ring 2  the blocks of neither with gap^2 < far2_hd[qb] = 1.0001 B_hd and fe_min[rb] < fe_max[qb], B_hd the largest hd_d2
          of the block's rows after ring 1 (+inf where a row has none).
Here everything is formed in float64 from the order: the float d2 of the device differs from float64 by at most
1.54e-5 at 256 columns, the margin is 1.0001 and the roundings of the gap are a few 2^-24, so with f_lo = 1 - 2e-5 and
f_hi = 1.001
  S1_lo = seed + {G < f_lo B_nn},  S1_hi = seed + {G < f_hi B_nn}            (B_nn over the seed references only)
  lower = S1_lo + {G < f_lo B_hd(S1_hi), fe_min < fe_max},  upper = S1_hi + {G < f_hi B_hd(S1_lo), fe_min < fe_max}
(B_hd(S): over the block's rows, the largest of the least d2 to a reference of lower free energy inside S) and the
`tiles` counter of a call lies in [16 |lower|, 16 |upper|], its `mfmas` counter is tiles x ceil((2 + 3 D) / 16)."""
import functools

import numpy as np

import widepruneref as pr

F32 = np.float32
BLOCK = pr.BLOCK
F_LO, F_HI = 1.0 - 2.0e-5, 1.001
FLT_MAX = np.finfo(np.float32).max

# rows x columns -> (evaluated block pairs, all block pairs) of widepruneref.stretched with the free energies of the
# populations at radii_for(D, 3)[0], under the numpy cell order: lower == upper at every shape
STRETCHED_TABLE = {(700, 100): (30, 36), (1500, 100): (86, 144), (2100, 100): (146, 289), (8320, 80): (1623, 4225)}
CONSTANT_2100 = 119   # 2100 x 100 under constant free energies: ring 2 is empty, the population sweep's count
GRADIENT_2100 = 124   # 2100 x 100 under fe = column 0


def mfmas_per_tile_pair(n_cols):
    return (2 + 3 * n_cols + 15) // 16


def seed_blocks(qb, nb):
    return [b for b in (qb - 1, qb, qb + 1) if 0 <= b < nb]


def _block_minima(c, fe, perm, qb):
    """float64 [rows of block qb][blocks]: the least d2 from each row of the block to the rows of every block (the row
    itself left out), and the same over the rows of lower free energy (IEEE comparison); +inf where there is none"""
    perm = np.asarray(perm, dtype=np.int64)
    n, nb = len(perm), pr.n_blocks(len(perm))
    x = c[perm].astype(np.float64)
    f = np.asarray(fe, dtype=np.float32)[perm]
    lo, hi = BLOCK * qb, min(BLOCK * (qb + 1), n)
    q = x[lo:hi]
    g = (x * x).sum(axis=1)
    d2 = np.maximum(g[lo:hi, None] + g[None, :] - 2.0 * (q @ x.T), 0.0)
    # (the Gram form loses digits where d2 is tiny against the norms: the pairs that matter are re-formed directly)
    near = d2 < 1e-6 * (g[lo:hi, None] + g[None, :])
    for i, j in zip(*np.nonzero(near)):
        d2[i, j] = ((q[i] - x[j]) ** 2).sum()
    d2[np.arange(hi - lo), np.arange(lo, hi)] = np.inf
    with np.errstate(invalid="ignore"):
        lower = f[None, :] < f[lo:hi, None]
    d2h = np.where(lower, d2, np.inf)
    pad = nb * BLOCK - n
    if pad:
        d2 = np.concatenate([d2, np.full((hi - lo, pad), np.inf)], axis=1)
        d2h = np.concatenate([d2h, np.full((hi - lo, pad), np.inf)], axis=1)
    return d2.reshape(hi - lo, nb, BLOCK).min(axis=2), d2h.reshape(hi - lo, nb, BLOCK).min(axis=2)


def _bound(minima, blocks):
    """the largest, over the rows, of the least entry inside the given blocks (a boolean mask); +inf if a row has none"""
    if not blocks.any():
        return np.inf
    return float(minima[:, blocks].min(axis=1).max())


def fe_ranges(fe, perm):
    """float64 [blocks][2]: (fe_min, fe_max) of every block of the order"""
    f = np.asarray(fe, dtype=np.float32)[np.asarray(perm, dtype=np.int64)].astype(np.float64)
    nb = pr.n_blocks(len(f))
    return np.array([(f[BLOCK * b:BLOCK * (b + 1)].min(), f[BLOCK * b:BLOCK * (b + 1)].max()) for b in range(nb)])


def block_sets(c, fe, perm, qb, boxes=None, ranges=None):
    """(seed, S1_lo, S1_hi, lower, upper) of query block qb: boolean masks over the reference blocks"""
    nb = pr.n_blocks(len(perm))
    boxes = pr.block_boxes(c, perm) if boxes is None else boxes
    ranges = fe_ranges(fe, perm) if ranges is None else ranges
    gap = pr.box_gap2(boxes[qb:qb + 1], boxes)[0]
    nn_min, hd_min = _block_minima(c, fe, perm, qb)
    seed = np.zeros(nb, dtype=bool)
    seed[seed_blocks(qb, nb)] = True
    b_nn = _bound(nn_min, seed)
    with np.errstate(invalid="ignore"):
        s1_lo = seed | (gap < F_LO * b_nn)
        s1_hi = seed | (gap < F_HI * b_nn)
        fe_ok = ranges[:, 0] < ranges[qb, 1]
        lower = s1_lo | ((gap < F_LO * _bound(hd_min, s1_hi)) & fe_ok)
        upper = s1_hi | ((gap < F_HI * _bound(hd_min, s1_lo)) & fe_ok)
    return seed, s1_lo, s1_hi, lower, upper


_COUNTS = {}


def block_counts(c, fe, perm):
    """int64 [blocks][4]: (|lower|, |upper|, |S1_lo|, |S1_hi|) of every query block; computed once per (data, order)"""
    perm = np.ascontiguousarray(perm, dtype=np.int64)
    key = (c.shape, hash(c.tobytes()), hash(np.ascontiguousarray(fe, dtype=np.float32).tobytes()), hash(perm.tobytes()))
    if key not in _COUNTS:
        boxes, ranges = pr.block_boxes(c, perm), fe_ranges(fe, perm)
        out = np.zeros((pr.n_blocks(len(c)), 4), dtype=np.int64)
        for qb in range(len(out)):
            _, s1_lo, s1_hi, lower, upper = block_sets(c, fe, perm, qb, boxes, ranges)
            out[qb] = (lower.sum(), upper.sum(), s1_lo.sum(), s1_hi.sum())
        _COUNTS[key] = out
    return _COUNTS[key]


def pair_bounds(c, fe, perm, segment=0, n_segments=0):
    """(|lower|, |upper|, |S1_lo|, |S1_hi|) in block pairs over the query blocks of a call"""
    qb = list(pr.segment_blocks(len(c), segment, n_segments))
    return tuple(int(v) for v in block_counts(c, fe, perm)[qb].sum(axis=0)) if qb else (0, 0, 0, 0)


def tile_bounds(c, fe, perm, segment=0, n_segments=0):
    """(lower, upper) for the `tiles` counter of a call: 16 tile pairs per evaluated block pair"""
    lo, hi, _, _ = pair_bounds(c, fe, perm, segment, n_segments)
    return 16 * lo, 16 * hi


def std_radius(n_cols):
    return pr.radii_for(n_cols, 3)[0]


@functools.lru_cache(maxsize=None)
def stretched_case(n_rows, n_cols):
    """(coords, free energies of the populations at radii_for(D, 3)[0], neighbours): once per shape"""
    from oracle.oracle import Oracle
    o = Oracle()
    c = pr.stretched(n_rows, n_cols)
    fe = o.free_energies(o.populations(c, [std_radius(n_cols)])[0])
    return c, fe, o.nearest_neighbors(c, fe)


@functools.lru_cache(maxsize=None)
def cross_block_tie_case(n_cols=100, seed=9):
    """-> (coords, fe, (a, p, q)): 384 rows in three groups that the order puts into one block each, by column 0.
    Row a lies at (0, 0) in the middle group; p at (-3, 0), a HIGH row index, in the block the order puts first; q at
    (+3, 0), a LOW row index, in the last block; a, p and q are equal in every other column, every other row is further
    than 9 from a, and fe[p] = fe[q] < fe[a]: d2(a, p) = d2(a, q) = 9 exactly, in every summation order, and the
    lexicographic minimum of (d2, ROW) is q both for nn and for hd.  A merge on positions would answer p."""
    from clustering_amd.synth import gaussian_blobs
    n = 3 * BLOCK
    c = gaussian_blobs(n, n_cols, seed=seed, sigma=0.5)   # (the other columns keep every other row further than 9 from a)
    rng = np.random.default_rng(seed + 1)
    # the groups by row index mod 3: first block rows 2 mod 3, middle 1 mod 3, last 0 mod 3 (interleaved: the order sorts
    # them); column 1 spans 0.1, so the cells are about 1 wide in column 0 and the groups, 1.5 apart, share none
    first, middle, last = np.arange(2, n, 3), np.arange(1, n, 3), np.arange(0, n, 3)
    c[first, 0] = rng.uniform(-16.0, -4.0, BLOCK).astype(F32)
    c[middle, 0] = rng.uniform(-1.5, 1.5, BLOCK).astype(F32)
    c[last, 0] = rng.uniform(4.0, 16.0, BLOCK).astype(F32)
    c[:, 1] = rng.uniform(-0.05, 0.05, n).astype(F32)
    a, p, q = int(middle[40]), int(first[120]), int(last[3])
    assert q < a < p
    base = c[a].copy()
    base[0], base[1] = 0.0, 0.0
    for r in (a, p, q):
        c[r] = base
    # p closes its block at column 0 = -3 and q opens its block at +3
    c[p, 0], c[q, 0] = F32(-3.0), F32(3.0)
    fe = rng.uniform(1.0, 2.0, n).astype(F32)
    fe[a], fe[p], fe[q] = F32(0.75), F32(0.5), F32(0.5)
    return np.ascontiguousarray(c), np.ascontiguousarray(fe), (a, p, q)


MARGIN_FAR2 = F32(1.0001) * F32(9.0)   # far2_nn of the margin cases' query block: its bound is the pair (a, a') at d2 = 9


def _gap_step(target):
    """a float dy with fl(9 + fl(dy * dy)) == target, for a float target a little above 9"""
    dy = F32(np.sqrt(float(target) - 9.0))
    for _ in range(64):
        got = F32(F32(9.0) + F32(dy * dy))
        if got == target:
            return dy
        dy = np.nextafter(dy, F32(1.0) if got < target else F32(0.0))
    raise AssertionError("no such step")


@functools.lru_cache(maxsize=None)
def margin_case(which, n_cols=80, seed=3):
    """-> (coords, fe, (a, a2), gap2): widepruneref.margin_case's construction with a block between, so that the far
    block is no seed block of the query block.  384 rows in three groups that the order puts into one block each, by
    column 0 (column 1 spans 0.1, the cells are narrower than the gaps between the groups):
      A (block 0): column 0 <= 0, column 1 <= 0; row a at (0, 0) and a2 at (-3, 0), equal in every other column, every
        other row of A an exact duplicate of another and far from a: the largest nn_d2 of the block after the seed is
        d2(a, a2) = 9 exactly -- a pair INSIDE the query block fixes far2_nn[0] = fl(1.0001f * 9) = MARGIN_FAR2;
      M (block 1): column 0 in [1.2, 1.8], duplicates, far from a in the other columns;
      B (block 2): column 0 >= 3 with a row at 3, column 1 >= dy with a row at dy, duplicates (far2_nn[2] is the
        floor: block 0 is in no ring of block 2).
    The box gap of blocks 0 and 2 is fl(9 + fl(dy^2)), and dy is chosen such that it is one ulp inside MARGIN_FAR2
    (which = -1), on it (0), one ulp outside (+1).  Constant free energies: ring 2 is empty."""
    from clustering_amd.synth import gaussian_blobs
    n = 3 * BLOCK
    half = gaussian_blobs(n // 2, n_cols, seed=seed, sigma=0.5)
    c = np.repeat(half, 2, axis=0)          # rows 2k and 2k + 1 are duplicates
    rng = np.random.default_rng(seed + 1)
    grp = [np.arange(g, n, 6)[:, None] + np.array([0, 1]) for g in (0, 2, 4)]   # pairs (6k + g, 6k + g + 1): interleaved groups
    A, M, B = (g.reshape(-1) for g in grp)
    target = MARGIN_FAR2 if which == 0 else np.nextafter(MARGIN_FAR2, F32(0.0) if which < 0 else F32(100.0))
    dy = _gap_step(target)
    pair = lambda lo, hi: np.repeat(rng.uniform(lo, hi, BLOCK // 2).astype(F32), 2)
    c[A, 0], c[A, 1] = pair(-6.0, -0.7), pair(-0.05, -0.001)
    c[M, 0], c[M, 1] = pair(1.2, 1.8), pair(-0.05, 0.05)
    c[B, 0], c[B, 1] = pair(3.5, 6.0), pair(0.04, 0.05)
    assert float(dy) < 0.04
    a, a2 = int(A[34]), int(A[35])
    c[a, 0], c[a, 1] = 0.0, 0.0
    c[a2] = c[a]
    c[a2, 0] = F32(-3.0)
    c[B[10:12], 0] = F32(3.0)
    c[B[20:22], 1] = dy
    return np.ascontiguousarray(c), np.zeros(n, dtype=np.float32), (a, a2), float(target)
