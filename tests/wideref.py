"""Case generators of the wide matrix-core sweeps' tests (65..256 columns): tests/test_wide_mfma_cases.py checks their
conditions on the CPU, tests/test_gpu_wide_mfma.py runs them on the device.

The band the kernel uses comes from the product's own host functions (pick_scale_nn, guard_e0, guard_kappa through
wide_band, dc_mfma_wide_kernels.hpp), asked of clustering_amd/bin/test_wide_model --band: no device is touched."""
import os
import subprocess

import numpy as np

from clustering_amd.synth import gaussian_blobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

COLS = (65, 80, 84, 85, 127, 128, 129, 255, 256)   # 84 | 85: 16 | 17 MFMAs, the seam of the 4-MFMA LDS chunk (63, 64, 65 slots
                                                   # past a chunk's end lie around 80 / 85 / 127 / 128 as well)
ROWS = (1, 2, 31, 32, 33, 97, 1500, 2100)            # 1 500: 12 x 12 blocks in one reference share; 2 100: 17 blocks, two shares
BOUNDARY_RADIUS = 3.0


def band(n_cols, coords):
    """(S, e0, kappa): the scale of the wide sweeps for this data and their band |acc - S d2| <= e0 + kappa S d2"""
    c = np.asarray(coords, dtype=np.float32)
    mu = (c.astype(np.float64).sum(axis=0) / len(c)).astype(np.float32)
    m = float((((c - mu).astype(np.float32).astype(np.float64)) ** 2).sum(axis=1).max()) * (1.0 + 4e-7)
    exe = os.path.join(ROOT, "clustering_amd", "bin", "test_wide_model")
    out = subprocess.run([exe, "--band", str(n_cols), repr(m)], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    assert out[0] == "band" and int(out[1]) == n_cols
    return float(out[2]), float(out[3]), float(out[4])


def eps(n_cols, coords, r2):
    """half-width of the undecided window around the squared radius r2, in the data's units"""
    s, e0, kappa = band(n_cols, coords)
    return (e0 + kappa * s * r2) / s


def blobs(n_rows, n_cols, seed=7):
    return gaussian_blobs(n_rows, n_cols, seed=seed)


def _free_rows(n_rows, used, wanted):
    """the wanted row numbers (mod n_rows), each moved up to the next row not in ``used``; adds them to ``used``"""
    out = []
    for r in wanted:
        r %= n_rows
        while r in used:
            r = (r + 1) % n_rows
        used.add(r)
        out.append(r)
    return out


def boundary_case(n_rows, n_cols, seed=3):
    """-> (coords, r, groups): blob frames, and in them groups of four rows (a, b, c, d) that differ in columns 0 / 1 only:
    d2(a, b) = 9 = fl32(r * r) exactly, d2(a, c) = 9 + ulp, d2(a, d) = 9 - ulp -- in every summation order, the sums
    having one or two non-zero terms.  The rows of a group lie in different tiles where n_rows allows."""
    assert n_rows >= 12
    c = gaussian_blobs(n_rows, n_cols, seed=seed, sigma=0.3)
    used, groups = set(), []
    for a in (0, n_rows // 3, n_rows - 4):
        rows = _free_rows(n_rows, used, [a, a + 37, a + 2 * n_rows // 3 + 1, a + n_rows // 2 + 2])
        base = c[rows[0]].copy()
        base[0], base[1] = 0.0, 0.0
        for r in rows:
            c[r] = base
        c[rows[1], 0] = F32(3.0)
        c[rows[2], 0], c[rows[2], 1] = F32(3.0), F32(2.0 ** -10)
        c[rows[3], 0] = F32(3.0) - F32(2.0 ** -22)
        groups.append(rows)
    return np.ascontiguousarray(c), BOUNDARY_RADIUS, groups


def ties_case(n_rows, n_cols, seed=5):
    """-> (coords, stars, dups): blob frames with (i) stars (centre, ring): a centre row and four rows at exactly the
    same distance from it (steps of 2^-6 along columns 0 / 1, both signs), closer than anything else, at scattered
    indices -- the lowest index must win; (ii) dups (copy, original): duplicate rows, d2 = 0 between them."""
    assert n_rows >= 24
    c = gaussian_blobs(n_rows, n_cols, seed=seed)
    step = F32(2.0 ** -6)
    used, stars, dups = set(), [], []
    for q0 in (n_rows // 5, n_rows // 2 + 1):
        q, *ring = _free_rows(n_rows, used, [q0, q0 + 3, q0 + n_rows // 3, q0 + n_rows // 3 + 1, q0 - 2])
        base = c[q].copy()
        base[0], base[1] = F32(1.0), F32(-0.5)   # (multiples of the step: the differences below are exact)
        c[q] = base
        for k, r in enumerate(ring):
            c[r] = base
            c[r, k // 2] += step if k % 2 == 0 else -step
        stars.append((q, ring))
    for k in range(3):
        copy, orig = _free_rows(n_rows, used, [7 * k + 1, n_rows - 1 - 5 * k])
        c[copy] = c[orig]
        dups.append((copy, orig))
    return np.ascontiguousarray(c), stars, dups


# ---- free energies for the neighbour sweeps ------------------------------------------------------------------------
def fe_all_equal(n):
    return np.full(n, 1.25, dtype=np.float32)


def fe_with_ties(n, seed=11):
    return np.random.default_rng(seed).integers(0, 4, n).astype(np.float32) * F32(0.5)


def fe_signed_zeros(n, seed=12):
    """+0.0, -0.0 (equal under the IEEE comparison the sweeps use) and a few values on either side"""
    v = np.random.default_rng(seed).choice(np.array([0.0, -0.0, -0.0, 0.0, 1.0, -1.0], dtype=np.float32), n)
    return np.ascontiguousarray(v, dtype=np.float32)


def fe_families(n):
    return {"equal": fe_all_equal(n), "ties": fe_with_ties(n), "zeros": fe_signed_zeros(n)}
