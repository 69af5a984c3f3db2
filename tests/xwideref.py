"""Cases of the matrix-core sweeps for rows of 257..1024 columns and the rules their tests rest on, restated in Python:
tests/test_xwide_cases.py checks the premises on the CPU, tests/test_gpu_xwide.py runs the cases on the device.

The generators are those of tests/wideref.py (blobs, boundary_case, ties_case, the free-energy families).  The rules --
nm_for, wide_shares, pick_scale_nn, guard_e0, guard_kappa, wide_window -- are restatements of dc_mfma_kernels.hpp and
dc_mfma_wide_kernels.hpp; test_xwide_cases.py holds them to the product's own host code where a binary prints it."""
import functools
import math

import numpy as np

import wideref
from wideref import blobs, boundary_case, fe_families, ties_case  # noqa: F401  (the cases' generators)

F32 = np.float32
U = 2.0 ** -24

# 257 -> 49 MFMAs (NM mod 4 = 1, the old maximum), 258 the same, 261 -> 50 (the first NM beyond it, mod 4 = 2), 267 -> 51,
# 272 -> 52 (mod 4 = 0); 341: the last column count of 64 MFMAs + 1; 400 | 401: the direct fallback's generic | column-chunked
# kernel; 512; 1023 | 1024: 192 | 193 MFMAs, the maximum
COLS = (257, 258, 261, 267, 272, 341, 400, 401, 512, 1023, 1024)
ROWS = (1, 2, 31, 32, 33, 127, 128, 129, 300, 1500, 2100)   # 1 500: 12 blocks, one reference share; 2 100: 17 blocks, two shares
MIN_COLS, MAX_COLS = 257, 1024
BAND_COLS = (257, 1024)   # the widths of the exact-path caps
BAND_ROWS = 1500
BLOCK_ROWS, BLOCK_TILES, KC = 128, 4, 4
MAX_SHARES, SHARE_BLOCKS = 64, 8
ROUND_MARGIN = 6.0e-7     # kWideRoundMargin


def nm_for(n_cols):
    """MFMAs per chain: three piece products per column and the two constant slots, 16 K slots per MFMA"""
    return (3 * n_cols + 2 + 15) // 16


def shares(ref_blocks):
    """wide_shares: a power of two, at most 64, and no more than leave every share 8 reference blocks"""
    s = 1
    while 2 * s <= MAX_SHARES and 2 * s * SHARE_BLOCKS <= ref_blocks:
        s *= 2
    return s


def blocks(n_rows):
    return (n_rows + BLOCK_ROWS - 1) // BLOCK_ROWS


def tile_pairs(n_query_blocks, n_ref_blocks):
    """32 x 32 tile pairs of an unpruned sweep: every query block meets every reference block, 4 x 4 tiles each -- in any
    number of shares, which split the reference blocks among workgroups and leave their number alone"""
    return n_query_blocks * n_ref_blocks * BLOCK_TILES * BLOCK_TILES


# ---- scale and band (dc_mfma_kernels.hpp pick_scale_nn, guard_e0, guard_kappa; dc_mfma_wide_kernels.hpp wide_window) ----------
def pick_scale_nn(m):
    """S = 2^(2k) with S M in [2^26, 2^28) (frexp: M = f 2^e, f in [0.5, 1); k = floor((28 - e) / 2), clamped)"""
    e = math.frexp(float(F32(m)))[1]
    k = max(-62, min(62, (28 - e) >> 1))
    return 2.0 ** (2 * k)


def nb_ns(n_cols):
    nb = (n_cols + 2 + 15) // 16
    return nb, nm_for(n_cols) - nb


def guard_e0(sm, n_cols, g=0, a=15):
    """the absolute part of the band at threshold 0, scaled extent sm = S M, the neighbour scale (g = 0, a = 15, c a power
    of two): guard_e0_linear + guard_flush"""
    nb, ns = nb_ns(n_cols)
    c_m = 3.0 + 4.1 + 27.0 + 34.0 + 72.4 * (nb - 1) + 0.072 * ns + 2.0
    flush = 2.0 ** (-12 - g) * math.sqrt(n_cols * sm) + 2.0 ** (-14 + a)
    return 1.25 * U * c_m * sm + 1.25 * flush


def guard_kappa(n_cols):
    nb, ns = nb_ns(n_cols)
    return 1.25 * U * (18.0 * ns + 1.0 + 0.25 * n_cols + 9.0)


def data_extent(coords):
    """M as the statistics pass forms it: the largest |x - mean|^2 over the float means, with its rounding margin"""
    c = np.asarray(coords, dtype=np.float32)
    mu = (c.astype(np.float64).sum(axis=0) / len(c)).astype(np.float32)
    return float(F32(float((((c - mu).astype(np.float32).astype(np.float64)) ** 2).sum(axis=1).max())) * F32(1.0 + 4e-7))


def band(n_cols, coords):
    """(S, e0, kappa) of the sweeps for this data: |acc - S d2| <= e0 + kappa S d2"""
    m = data_extent(coords)
    s = pick_scale_nn(m)
    return s, guard_e0(float(F32(m) * F32(s)), n_cols), guard_kappa(n_cols)


def window_margin(thr, e0):
    """wide_window's allowance for its own float roundings"""
    return (thr + e0) * ROUND_MARGIN


# ---- the exact-path cap of the population sweep ------------------------------------------------------------------------------
def pair_d2(coords):
    """float64 squared distances of all ordered pairs, the diagonal included"""
    x = np.asarray(coords, dtype=np.float64)
    g = (x * x).sum(axis=1)
    return np.maximum(g[:, None] + g[None, :] - 2.0 * (x @ x.T), 0.0)


@functools.lru_cache(maxsize=None)
def band_case(n_cols):
    """-> (coords, radii, bound, pairs): the 1 500-row blob case of one width, its radii at the 25 % and 5 % quantiles of the
    pair distances, and the cap on the pairs a correct population sweep can send to the exact path: an accumulator lies
    within e0 + kappa S d2 of S d2 and is undecided within e0 + kappa t (+ the window's margin) of a threshold t = S fl32(r^2),
    so only pairs with |S d2 - t| <= 2 (e0 + kappa t) + margin can be deferred -- counted here in float64 over the ordered
    pairs i != j (the sweep meets a pair from both ends), a pair near both radii once -- plus the pairs exactly at a radius.
    The bound is first-order: the accumulator's own error is e0 + kappa S d2, not kappa t, so just above a threshold the true
    set is wider by kappa times the band, 2e-4 of it at most -- against which the sweep reads half the bound.
    pairs: n (n - 1), what the bound is a share of."""
    c = blobs(BAND_ROWS, n_cols)
    d2 = pair_d2(c)
    off = ~np.eye(len(c), dtype=bool)
    radii = [float(np.sqrt(np.quantile(d2[off], 0.25))), float(np.sqrt(np.quantile(d2[off], 0.05)))]
    s, e0, kappa = band(n_cols, c)
    near = np.zeros_like(off)
    at = 0
    for r in radii:
        r2 = float(F32(r) * F32(r))
        t = s * r2
        near |= np.abs(s * d2 - t) <= 2.0 * (e0 + kappa * t) + window_margin(t, e0)
        at += int(((d2 == r2) & off).sum())
    return c, radii, int((near & off).sum()) + at, len(c) * (len(c) - 1)
