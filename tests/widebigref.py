"""Case generators and referees of the wide matrix-core sweeps (65..256 columns) at the sizes they were written for:
many reference shares, more than one launch group, queues that fill, degenerate statistics.  tests/test_wide_big_cases.py
checks their conditions on the CPU, tests/test_gpu_wide_big.py runs them on the device.  The unit map and the share
counts come from the product's own functions (wide_unit, wide_grid_size, wide_shares of dc_mfma_wide_kernels.hpp), asked
of clustering_amd/bin/test_wide_model --units / --shares: no device is touched.  Importing this module needs neither a
GPU nor torch."""
import functools
import os
import subprocess

import numpy as np

import wideref
from clustering_amd.synth import gaussian_blobs
from crossref import block_d2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
BLOCK = 128          # kWideBlockRows: rows of a query block and of a reference block
MAX_SHARES = 64      # kWideShares
GROUP = 512          # workgroups of one launch group (wide_grid_size)
QUEUE = 256          # kWideQueue: deferred pairs a wave parks before it drains them inside push
STEP = F32(2.0 ** -6)
TIE_D2 = F32(2.0 ** -12)


def _model(*args):
    exe = os.path.join(ROOT, "clustering_amd", "bin", "test_wide_model")
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120, check=True).stdout


def blocks(n_rows):
    return (n_rows + BLOCK - 1) // BLOCK


@functools.lru_cache(maxsize=None)
def shares(ref_blocks):
    """wide_shares(ref_blocks), from the product"""
    out = _model("--shares", ref_blocks).split()
    assert out[0] == "shares" and int(out[1]) == ref_blocks
    return int(out[2])


def shares_of_rows(n_ref):
    return shares(blocks(n_ref))


def units(n_shares, q_blocks):
    """-> (grid, [grid, 2] array of (q_block, share) per workgroup id): wide_grid_size and wide_unit, from the product"""
    lines = _model("--units", n_shares, q_blocks).split("\n")
    head = lines[0].split()
    assert head[0] == "grid"
    grid = int(head[1])
    tab = np.array([ln.split() for ln in lines[1:] if ln], dtype=np.int64)
    assert tab.shape == (grid, 3) and (tab[:, 0] == np.arange(grid)).all()
    return grid, tab[:, 1:]


def swept_units(n_ref, lo, hi):
    """(query block, share) units a launch over the query rows [lo, hi) really sweeps"""
    return ((hi + BLOCK - 1) // BLOCK - lo // BLOCK) * shares_of_rows(n_ref)


def place(row, n_shares):
    """where the sweep meets reference row `row`: (block, share, wr, half) -- the block's share, the pair of waves that
    holds its tile (tiles 0-1: wr 0, tiles 2-3: wr 1) and the half of the wave (dc_credit.hpp tile_row_local: the rows
    4..7, 12..15, ... of a tile sit in the lanes 32..63)"""
    b = row // BLOCK
    return b, b % n_shares, (row % BLOCK) // 64, ((row % 32) >> 2) & 1


# ---- referees -----------------------------------------------------------------------------------------------------------
def rect_d2(probe, Q, R, chunk=1024):
    """the probe's canonical d2 of every (query, reference) pair, tiled over BOTH sets: the probe evaluates the whole
    union of what it is given, so a long Q is cut as well as a long R (the d2 of a pair depends on its two rows alone).
    A short Q meets pieces of R of its own length: the union of two equal pieces wastes the least."""
    n_q, n_r = len(Q), len(R)
    out = np.empty((n_q, n_r), dtype=np.float32)
    for a in range(0, n_q, chunk):
        q = Q[a:a + chunk]
        step = max(min(chunk, len(q)), 64)
        for b in range(0, n_r, step):
            out[a:a + chunk, b:b + step] = block_d2(probe, q, R[b:b + step])
    return out


# ---- ties whose tied references lie in different shares, waves and halves -----------------------------------------------------
def star_across_shares(R_rows, n_cols, n_shares, self_form=False, seed=5):
    """-> dict(R, stars, dup, fe_r, n_shares): blob frames with two stars and a duplicate pair, placed by block arithmetic.

    A star is a centre and six ring rows at exactly d2 = 2^-12 from it (the construction of wideref.ties_case: steps of
    2^-6 along columns 0, 1, 2, both signs, from a base whose first columns are multiples of the step -- one non-zero
    term, the same in every summation order), closer than anything else.  With B the star's first block and S = n_shares:
        a = 128 B + 2           tile 0, first half of the wave      the LOWEST index
        b = 128 B + 5           tile 0, second half                 met before a: accumulator register 1, a is register 2
        c = 128 B + 64 + 9      the same block, tile 2: the other pair of waves (wr)
        d = 128 (B + S) + 40    the same share, a later block
        e = 128 (B + 1) + 77    another share
        f = 128 (B + S + 3) + 100   a third share
    star 0: every ring row lies below the centre's free energy: nn = nn_hd = a.
    star 1: a, b, c, d -- the whole of a's share -- lie ABOVE it and e, f below: nn = a, nn_hd = e, from different shares.
    dup: (lo, hi), two equal rows in blocks of different shares and a centre that copies them: d2 = 0 twice, lo wins.

    stars: [(centre vector, ring rows a..f, fe of the centre)], dup: (centre vector, lo, hi, fe of the centre); fe_r:
    random free energies of R with the values the stars need.  self_form: the centres are rows of R too (the last whole
    blocks: rows `centres`, in one range `span` of three query blocks); otherwise they are meant for a query set
    (star_queries)."""
    S = n_shares
    RB = blocks(R_rows)
    assert S >= 4 and RB >= 4 * S + 16 and R_rows >= 128 * (RB - 1) + 64
    R = gaussian_blobs(R_rows, n_cols, seed=seed)
    rng = np.random.default_rng(seed + 1)
    fe_r = rng.normal(size=R_rows).astype(np.float32)
    stars = []
    for k, B in enumerate((3, 2 * S + 6)):
        ring = [128 * B + 2, 128 * B + 5, 128 * B + 64 + 9, 128 * (B + S) + 40, 128 * (B + 1) + 77, 128 * (B + S + 3) + 100]
        base = R[ring[0]].copy()
        base[0], base[1], base[2] = F32(1.0), F32(-0.5), F32(0.25)   # (multiples of the step: the differences below are exact)
        for m, r in enumerate(ring):
            R[r] = base
            R[r, m // 2] += STEP if m % 2 == 0 else -STEP
        fe_c = F32(0.5)
        fe_r[ring] = F32(0.25) - F32(0.01) * np.arange(6, dtype=np.float32)
        if k == 1:
            fe_r[ring[:4]] = F32(0.75)
        stars.append((base, ring, fe_c))
    lo, hi = 128 * (S + 2) + 33, 128 * (3 * S + 7) + 70
    R[hi] = R[lo]
    fe_r[[lo, hi]] = F32(-3.0)
    dup = (R[lo].copy(), lo, hi, F32(0.0))
    out = dict(R=R, stars=stars, dup=dup, fe_r=fe_r, n_shares=S)
    if self_form:
        first = 128 * (RB - 4)
        centres = [first + 17, first + 128 + 72, first + 256 + 5]
        used = set(r for _, ring, _ in stars for r in ring) | {lo, hi}
        assert not used & set(centres) and max(used) < first
        for row, (vec, fe_c) in zip(centres, [(s[0], s[2]) for s in stars] + [(dup[0], dup[3])]):
            R[row] = vec
            fe_r[row] = fe_c
        out.update(centres=centres, span=(first + 10, first + 300))
    out["R"] = np.ascontiguousarray(R)
    return out


def star_queries(case, n_q, n_cols, seed=9):
    """-> (Q, fe_q, rows): n_q blob queries with the centres of the case's stars and of its duplicate pair at `rows`"""
    Q = gaussian_blobs(n_q, n_cols, seed=seed)
    fe_q = np.random.default_rng(seed + 1).normal(size=n_q).astype(np.float32)
    rows = [2, n_q // 2 + 1, n_q - 1]
    for row, (vec, fe_c) in zip(rows, [(s[0], s[2]) for s in case["stars"]] + [(case["dup"][0], case["dup"][3])]):
        Q[row] = vec
        fe_q[row] = fe_c
    return np.ascontiguousarray(Q), fe_q, rows


# ---- a scale set by a few far rows: every cluster pair inside the band of every radius -----------------------------------
OUTLIER_L = 100.0
OUTLIER_D2 = 0.05   # 2 sigma^2 D, the mean intra-cluster d2


def outlier_case(n_cluster, n_cols, seed=21):
    """-> dict(c, radii, Q, R, n_cluster): a tight Gaussian cluster (rows 0 .. n_cluster - 1, 2 sigma^2 D = 0.05) and two
    rows at +L and -L along column 0, L = 100: symmetric, so the mean stays in the cluster and M ~ L^2.  The band of the
    sweeps is a fraction of M (eps ~ 3e-5 L^2 = 0.3 at 65 columns), the cluster's d2 spread over a few hundredths: every
    cluster pair is undecided at every radius near the cluster's own d2.  radii: eight, at the median and seven other
    quantiles of the intra-cluster d2, not sorted -- eight flags in one queue entry, and exact decisions that differ.
    Q, R: a cross split of the same rows (Q: 200 cluster rows and the row at +L; R: the rest and the row at -L)."""
    rng = np.random.default_rng(seed)
    sigma = np.sqrt(OUTLIER_D2 / (2.0 * n_cols))
    c = rng.normal(0.0, sigma, (n_cluster + 2, n_cols))
    c[:, 0] += 0.5   # (off the origin: the mean is not zero)
    c[n_cluster], c[n_cluster + 1] = c[0], c[1]
    c[n_cluster, 0] += OUTLIER_L
    c[n_cluster + 1, 0] -= OUTLIER_L
    c = np.ascontiguousarray(c.astype(np.float32))
    x = c[:n_cluster].astype(np.float64)
    g = (x * x).sum(axis=1)
    d2 = (g[:, None] + g[None, :] - 2.0 * (x @ x.T))[np.triu_indices(n_cluster, 1)]
    radii = [float(np.sqrt(np.quantile(d2, q))) for q in (0.5, 0.1, 0.9, 0.3, 0.7, 0.2, 0.8, 0.6)]
    n_q = min(200, n_cluster // 2)
    Q = np.ascontiguousarray(np.vstack([c[:n_q], c[n_cluster:n_cluster + 1]]))
    R = np.ascontiguousarray(np.vstack([c[n_q:n_cluster], c[n_cluster + 1:]]))
    return dict(c=c, radii=radii, Q=Q, R=R, n_cluster=n_cluster)


# ---- degenerate statistics ------------------------------------------------------------------------------------------------
DEGENERATE_RADII = [0.0, 1e-30, 1.0, 5.0, 1e15, 1e30]   # fl32(r * r): 0, 0 (1e-60 underflows), 1, 25, 1e30, inf


def identical_rows(n, n_cols, one_ulp=False):
    """n copies of one blob row: M = max |x - mean|^2 is 0 or a few ulp^2, the scale exponent of pick_scale_nn far up, and
    a finite radius gives a scaled threshold beyond FLT_MAX.  one_ulp: column 7 of row n // 2 + 3 is the next float up."""
    row = gaussian_blobs(4, n_cols, seed=31)[1]
    c = np.tile(row, (n, 1))
    if one_ulp:
        c[n // 2 + 3, 7] = np.nextafter(c[n // 2 + 3, 7], F32(np.inf))
    return np.ascontiguousarray(c)


def extent(c):
    """M = max |x - mean|^2 as the statistics pass forms it (wideref.band): double column sums, a float mean"""
    c = np.asarray(c, dtype=np.float32)
    mu = (c.astype(np.float64).sum(axis=0) / len(c)).astype(np.float32)
    return float((((c - mu).astype(np.float32).astype(np.float64)) ** 2).sum(axis=1).max())


def fe_random(n, seed=17):
    """free energies of any origin: normal draws rounded to sixteenths, so that many tie"""
    return (np.round(np.random.default_rng(seed).normal(size=n) * 16.0) / 16.0).astype(np.float32)
