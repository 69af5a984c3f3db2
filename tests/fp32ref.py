"""The cases of tests/test_gpu_fp32.py (the fp32-input matrix-core sweeps for rows of 1..32 columns, several radii per
sweep) and what each is there for, as functions that tests/test_fp32_cases.py evaluates on the CPU: a case whose premise
stopped holding fails there instead of silently testing nothing on the GPU.

scale_pop() restates scale32_pop of clustering_amd/csrc/dc_mfma32_band.hpp in float64: S = c^2 is the factor between
data units and the units in which the sweep's guard band is 1."""
import functools

import numpy as np

from clustering_amd.synth import gaussian_blobs

COLS = (1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 16, 17, 21, 24, 25, 30, 31, 32)   # (21: the instances of 11 K-steps)
ROWS = (1, 32, 33, 257, 600, 3000)
U = 2.0 ** -24


def k_steps(n_cols):
    """K-steps of the kernel instance (dc_mfma32_general.hip fp32_steps): ceil(D / 2), the even counts below 16 one more"""
    s = (n_cols + 1) // 2
    return s + 1 if (s % 2 == 0 and s < 16) else s


def max_norm(c):
    """max |x - mean|^2 with the float32 means the library centres with (header word 0, to a few ulp)"""
    mu = c.astype(np.float64).mean(axis=0).astype(np.float32)
    x = (c - mu).astype(np.float64)
    return float((x * x).sum(axis=1).max())


def scale_pop(M, r2max, n_cols):
    """c of scale32_pop for the instance that serves n_cols"""
    K = 2 * k_steps(n_cols)
    eps1 = 1.25 * U * ((4.0 * K + 13.0) * M + (0.25 * n_cols + 18.0) * max(r2max, 0.0))
    if not eps1 > 1.0e-76:
        return 2.0 ** 63
    c = np.sqrt((1.0 - 1.0 / 65536.0) / eps1) * (1.0 - 1.0 / 1048576.0)
    return float(min(max(c, 2.0 ** -60), 2.0 ** 63))


def d2_all(c):
    x = c.astype(np.float64)
    g = (x * x).sum(axis=1)
    return np.maximum(g[:, None] + g[None, :] - 2.0 * x @ x.T, 0.0)


def d2_pair(c, i, j):
    x = c[i].astype(np.float64) - c[j].astype(np.float64)
    return float((x * x).sum())


@functools.lru_cache(maxsize=None)
def blobs(n_rows, n_cols, seed=11):
    """three gaussian blobs with duplicates planted: row 0 again in the last row and in the middle, a triple further on"""
    c = gaussian_blobs(n_rows, n_cols, seed=seed).astype(np.float32)
    if n_rows >= 3:
        c[n_rows - 1] = c[0]
        c[n_rows // 2] = c[0]
    if n_rows >= 40:
        c[35] = c[33]
        c[7] = c[33]
    c.setflags(write=False)
    return c


def radii_for(c, k=1):
    """k radii around the 10 % quantile of the pair distances of the first 64 rows, unsorted and distinct"""
    d2 = d2_all(c[:64])
    off = d2[np.triu_indices(len(d2), 1)]
    base = float(np.sqrt(np.quantile(off, 0.1))) if off.size and off.max() > 0 else 1.0
    base = base if base > 0 else 1.0
    return [base * f for f in (1.0, 0.8, 1.25, 0.9, 1.5, 0.7, 1.1, 0.6, 1.35, 0.95, 2.0, 0.5, 1.05, 0.75, 1.6, 0.85, 1.2)[:k]]


def radius_sets(c):
    """name -> radii: 1, 2, 3, 8 and 9 radii, unsorted, with an equal pair, with 0, +inf and NaN"""
    r = radii_for(c, 9)
    return {
        "one": r[:1],
        "two_descending": [r[2], r[1]],
        "three_unsorted": [r[0], r[2], r[1]],
        "three_equal_pair": [r[1], r[0], r[1]],
        "three_zero_inf_nan": [0.0, float("inf"), float("nan")],
        "eight_with_edges": [r[0], float("inf"), 0.0, r[3], float("nan"), r[5], r[0], r[4]],
        "nine": r,
    }


def lattice_case(n_cols, side=6):
    """points k / 2 on a grid in the first min(D, 3) columns and radius 1: pairs two steps apart along an axis have d^2
    exactly equal to r^2 and are NOT inside (strict <); every value is exact in float32"""
    dims = min(n_cols, 3)
    g = np.stack(np.meshgrid(*[np.arange(side)] * dims, indexing="ij"), axis=-1).reshape(-1, dims).astype(np.float32) * 0.5
    c = np.zeros((len(g), n_cols), dtype=np.float32)
    c[:, :dims] = g
    rng = np.random.default_rng(5)
    return np.ascontiguousarray(c[rng.permutation(len(c))]), [1.0, 0.5, 1.5]


def lattice_premise(c, radii):
    d2 = d2_all(c)
    return {float(r): int((d2 == float(np.float32(r)) ** 2).sum()) for r in radii}


def band_case(n_rows, n_cols):
    """blobs and three radii whose smallest and largest are the float32 distances of two chosen pairs: r^2 and that
    pair's d^2 differ by rounding alone, far less than the band -- only the exact re-check decides them"""
    c = blobs(n_rows, n_cols, seed=23)
    d2 = d2_all(c[:200])
    iu = np.triu_indices(len(d2), 1)
    order = np.argsort(d2[iu])
    order = order[d2[iu][order] > 0]
    near, far = order[len(order) // 50], order[len(order) // 4]
    pairs = [(int(iu[0][near]), int(iu[1][near])), (int(iu[0][far]), int(iu[1][far]))]
    r_near = float(np.float32(np.sqrt(d2_pair(c, *pairs[0]))))
    r_far = float(np.float32(np.sqrt(d2_pair(c, *pairs[1]))))
    return c, [r_far, 0.5 * (r_near + r_far), r_near], pairs


def band_premise(c, radii, pairs):
    """|S d^2 - S r^2| of the pair chosen for the smallest and for the largest radius, at the scale of the call"""
    r2max = float(np.float32(max(radii)) ** 2)
    S = scale_pop(max_norm(c), r2max, c.shape[1]) ** 2
    lo, hi = min(radii), max(radii)
    return (abs(S * d2_pair(c, *pairs[0]) - S * float(np.float32(lo)) ** 2),
            abs(S * d2_pair(c, *pairs[1]) - S * float(np.float32(hi)) ** 2))


def tie_case(n_cols):
    """600 rows of which every row of the second half repeats one of the first 40: equal distances whose lowest index wins"""
    c = np.array(blobs(600, n_cols, seed=31))
    rng = np.random.default_rng(9)
    c[300:] = c[rng.integers(0, 40, 300)]
    return np.ascontiguousarray(c)


def tile_test_case(n_cols, n_rows=600):
    """radii (tiny, huge): every pair of distinct rows lies outside the smallest radius by more than the band and inside
    the largest, so every chain that holds no row twice passes the tile test of the largest radius and fails that of the
    smallest, whatever order the sweep puts the rows in; populations differ between the two"""
    rng = np.random.default_rng(41)
    c = rng.uniform(-1.0, 1.0, (n_rows, n_cols)).astype(np.float32)
    d2 = d2_all(c)
    off = d2[np.triu_indices(n_rows, 1)]
    return c, [float(np.sqrt(off.min()) * 0.5), float(np.sqrt(off.max()) * 2.0)]


def tile_test_premise(c, radii):
    """(smallest scaled gap of a pair above the small radius, ... below the large one): both must exceed 2 (t >= 2: outside)"""
    d2 = d2_all(c)
    off = d2[np.triu_indices(len(c), 1)]
    lo, hi = float(np.float32(min(radii))) ** 2, float(np.float32(max(radii))) ** 2
    S = scale_pop(max_norm(c), hi, c.shape[1]) ** 2
    return S * (off.min() - lo), S * (hi - off.max())


def fuzz_shapes(count=40, seed=2026):
    """(n_rows, n_cols, n_radii, seed) of the fixed-seed fuzz against variant="direct\""""
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(1, 700)), int(rng.integers(1, 33)), int(rng.integers(1, 10)), int(rng.integers(0, 1 << 30)))
            for _ in range(count)]
