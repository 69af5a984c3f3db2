"""Case generators of the cross form of the wide matrix-core sweeps (65..256 columns, queries against a reference):
tests/test_cross_wide_cases.py checks their conditions on the CPU, tests/test_gpu_cross_wide.py runs them on the device.
Importing this module needs neither a GPU nor torch."""
import numpy as np

from clustering_amd.synth import gaussian_blobs

F32 = np.float32
BOUNDARY_RADIUS = 3.0


def nm_for(n_cols):
    """MFMAs of one chain (dc_mfma_kernels.hpp nm_for): two constant slots and three products per column, 16 slots each"""
    return (3 * n_cols + 2 + 15) // 16


def tile_pairs(n_q, n_r, lo=0, hi=None):
    """32x32 tile pairs one launch evaluates: whole 128-row blocks, the query blocks the rows [lo, hi) touch"""
    hi = n_q if hi is None else hi
    if hi <= lo or n_r == 0:
        return 0
    return 16 * ((hi + 127) // 128 - lo // 128) * ((n_r + 127) // 128)


def blob_sets(n_cols, n_q, n_r, seed=7, sigma=0.08):
    """queries and references from the same blobs, no frame twice"""
    c = gaussian_blobs(n_q + n_r, n_cols, seed=seed, sigma=sigma)
    return np.ascontiguousarray(c[:n_q]), np.ascontiguousarray(c[n_q:])


def radii_for(n_cols, k=3, sigma=0.08):
    """k radii around the intra-blob distance of synth.gaussian_blobs (d2 ~ 2 sigma^2 D), not sorted"""
    base = float(np.sqrt(2 * sigma * sigma * n_cols))
    return [base * f for f in (1.0, 0.9, 1.08, 0.95, 1.2, 0.8, 1.02, 0.85, 1.1)[:k]]


def boundary_sets(n_q, n_r, n_cols, seed=3):
    """-> (Q, R, r, groups): blob frames and groups (a, b, c, d) ACROSS the sets -- a a query row, b, c, d reference rows in
    three different 32-row tiles -- that differ in columns 0 / 1 only: d2(a, b) = 9 = fl32(r * r) exactly,
    d2(a, c) = 9 + ulp, d2(a, d) = 9 - ulp, in every summation order (the sums have one or two non-zero terms)."""
    assert n_q >= 12 and n_r >= 128
    Q, R = blob_sets(n_cols, n_q, n_r, seed=seed, sigma=0.3)
    groups = []
    for k, a in enumerate((1, n_q // 2, n_q - 2)):
        b, c, d = 3 + 5 * k, 32 + (n_r // 2 + 7 * k) % (n_r - 64), n_r - 1 - 9 * k
        assert len({b // 32, c // 32, d // 32}) == 3
        base = Q[a].copy()
        base[0], base[1] = 0.0, 0.0
        Q[a] = base
        for j in (b, c, d):
            R[j] = base
        R[b, 0] = F32(3.0)
        R[c, 0], R[c, 1] = F32(3.0), F32(2.0 ** -10)
        R[d, 0] = F32(3.0) - F32(2.0 ** -22)
        groups.append((a, b, c, d))
    return Q, R, BOUNDARY_RADIUS, groups


def ties_sets(n_q, n_r, n_cols, seed=5):
    """-> (Q, R, stars, copies, twins): blob frames with
    stars  (q, ring): a query and four references at exactly the same distance from it (steps of 2^-6 along columns
           0 / 1, both signs), closer than anything else, at scattered indices not met in index order;
    copies (q, j): a query that is a copy of reference j (d2 = 0), j the only such row;
    twins  (q, j_low, j_high): two equal reference rows and a query that copies them -- the lower index wins."""
    assert n_q >= 16 and n_r >= 160
    Q, R = blob_sets(n_cols, n_q, n_r, seed=seed)
    step = F32(2.0 ** -6)
    stars, copies, twins = [], [], []
    for k, q in enumerate((2, n_q // 2 + 1)):
        ring = [n_r - 3 - 11 * k, 37 + k, n_r // 2 + 5 * k, 70 + 3 * k]
        base = Q[q].copy()
        base[0], base[1] = F32(1.0), F32(-0.5)   # (multiples of the step: the differences below are exact)
        Q[q] = base
        for m, j in enumerate(ring):
            R[j] = base
            R[j, m // 2] += step if m % 2 == 0 else -step
        stars.append((q, ring))
    for k, q in enumerate((5, n_q - 1)):
        j = 90 + 13 * k
        Q[q] = R[j]
        copies.append((q, j))
    for k, q in enumerate((7, n_q // 3)):
        lo, hi = 9 + 40 * k, n_r - 20 - 2 * k
        R[hi] = R[lo]
        Q[q] = R[lo]
        twins.append((q, lo, hi))
    used = [j for _, ring in stars for j in ring] + [j for _, j in copies] + [j for _, lo, hi in twins for j in (lo, hi)]
    assert len(set(used)) == len(used) and len({q for q, *_ in stars + copies + twins}) == 6, "the constructions share a row"
    return Q, R, stars, copies, twins


def fe_pair(n_q, n_r, seed=17):
    """free energies of any origin for both sides: normal draws, a few exact ties between the sides"""
    rng = np.random.default_rng(seed)
    fq, fr = rng.normal(size=n_q).astype(np.float32), rng.normal(size=n_r).astype(np.float32)
    if n_q and n_r:
        fq[:: 5] = fr[rng.integers(0, n_r, len(fq[:: 5]))]
    return fq, fr


def offset_sets(n_cols, n_q, n_r, seed=7):
    """blob sets with the queries moved off by more than a blob distance (4 along column 2): no query has a reference
    inside a radius of radii_for, every nearest reference is far"""
    Q, R = blob_sets(n_cols, n_q, n_r, seed=seed)
    Q[:, 2] += F32(4.0)
    return np.ascontiguousarray(Q), R


FLAWS = ("nan query", "inf query", "nan reference", "inf reference", "big query", "big reference")


def flawed_sets(Q, R, flaw):
    """copies of (Q, R) with ONE row of one set that the statistics pass flags: a NaN, an inf, or a finite coordinate of
    2e18 (|x|^2 = 4e36 > 1e36, the sweeps' norm limit; its distances stay finite)"""
    Q, R = Q.copy(), R.copy()
    kind, side = flaw.split()
    X = Q if side == "query" else R
    row, col = len(X) // 2 + 3, X.shape[1] - 1
    X[row, col] = {"nan": np.nan, "inf": np.inf, "big": 2.0e18}[kind]
    return Q, R


def flawed_row(Q, R, flaw):
    return (len(Q) if flaw.endswith("query") else len(R)) // 2 + 3
