"""Case generators and the numpy order of the resident reference's tests (dc_hip_reference_wide_*, 65..256 columns,
DESIGN.md 4.28): tests/test_reference_wide_cases.py checks their premises on the CPU, tests/test_gpu_wide_reference.py
runs them on the device.  Importing this module needs neither a GPU nor torch.

What differs from the pruned cross sweeps (crosswidepruneref): origin, scale and grid come from the REFERENCE alone.
The origin is its column mean, the scale that of M_res = 4 M_ref (M_ref the largest |x - mean|^2 of the reference), the
grid its extent in columns 0 / 1 -- a query outside it is clamped to an edge cell."""
import os
import subprocess

import numpy as np

import crosswidepruneref as pr
import crosswideref as cw
from widepruneref import BLOCK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
HEADROOM = 4.0   # M_res / M_ref


def reference_order(Q, R, frames_per_cell=BLOCK):
    """both spatial orders as the resident reference builds them, in numpy: the cell grid on columns 0 / 1 over the finite
    entries of R ALONE, the cell sized for its row count, serpentine keys, key 0 for a non-finite row, the queries clamped
    to the grid, one stable sort per set.  -> (perm_q, perm_r), position -> row of the set"""
    U = R[:, :2].astype(np.float64)
    x, y = U[:, 0], U[:, 1]
    fx, fy = np.isfinite(x), np.isfinite(y)
    lo0, hi0 = (x[fx].min(), x[fx].max()) if fx.any() else (0.0, 0.0)
    lo1, hi1 = (y[fy].min(), y[fy].max()) if fy.any() else (0.0, 0.0)
    e0, e1 = hi0 - lo0, hi1 - lo1
    f = frames_per_cell / max(len(R), 1)
    cell = np.sqrt(e0 * e1 * f) if e0 > 0 and e1 > 0 else (e0 + e1) * f
    cell = max(cell, max(e0, e1) / 4000.0)
    if not cell > 0:
        cell = 1.0
    ny = int(min(e1 / cell, 4000.0)) + 1

    def order(A):
        ax, ay = A[:, 0].astype(np.float64), A[:, 1].astype(np.float64)
        ok = np.isfinite(ax) & np.isfinite(ay)
        bx = np.clip(np.where(ok, (ax - lo0) / cell, 0.0), 0.0, 4000.0).astype(np.int64)
        by = np.minimum(np.clip(np.where(ok, (ay - lo1) / cell, 0.0), 0.0, 4000.0).astype(np.int64), ny - 1)
        key = np.where(ok, bx * ny + np.where(bx & 1, ny - 1 - by, by), 0)
        return np.argsort(key, kind="stable")

    return order(Q), order(R)


def means(R):
    """the resident origin as the device forms it: double column sums, divided, rounded to float"""
    return (R.astype(np.float64).sum(axis=0) / len(R)).astype(F32)


def norms2(X, R):
    """float64 |x - mean(R)|^2 of every row of X, from the centred floats"""
    return ((X - means(R)).astype(F32).astype(np.float64) ** 2).sum(axis=1)


def m_ref(R):
    return float(norms2(R, R).max())


def outside_box(Q, R):
    """rows of Q whose column 0 or column 1 lies outside the reference's extent"""
    lo, hi = R[:, :2].min(axis=0), R[:, :2].max(axis=0)
    return ((Q[:, :2] < lo) | (Q[:, :2] > hi)).any(axis=1)


def ordinary_batch(R, n_q, seed=31):
    """n_q blob frames of the reference's distribution, none of them a reference row, all below 0.85 M_ref"""
    n_cols = R.shape[1]
    cand = cw.blob_sets(n_cols, 3 * n_q + 64, 8, seed=seed)[0]
    keep = cand[norms2(cand, R) < 0.85 * m_ref(R)]
    assert len(keep) >= n_q, "too few candidates inside the reference's extent"
    return np.ascontiguousarray(keep[:n_q])


def _moved(R, Q, rows, factor, planar):
    """Q with `rows` put at mean + d, |d|^2 = factor M_ref; planar: d in the (column 0, column 1) plane, a corner each"""
    Q, mu, m = Q.copy(), means(R).astype(np.float64), m_ref(R)
    for k, i in enumerate(rows):
        d = np.zeros(R.shape[1])
        if planar:
            d[0] = np.sqrt(0.5 * factor * m) * (1 if k & 1 else -1)
            d[1] = np.sqrt(0.5 * factor * m) * (1 if k & 2 else -1)
        else:
            d[2 + k % (R.shape[1] - 2)] = np.sqrt(factor * m)
        Q[i] = (mu + d).astype(F32)
    return np.ascontiguousarray(Q)


def headroom_batch(R, n_q, seed=31):
    """inside the headroom, outside the extent: an ordinary batch with a few rows at |x'|^2 = 2.2 M_ref on the four diagonals
    of the (column 0, column 1) plane -- each beyond the reference's box in both columns (|x_k - mean_k| <= sqrt(M_ref) for
    every reference row, these sit at sqrt(1.1 M_ref))"""
    rows = [0, n_q // 3, n_q // 2, n_q - 1] if n_q >= 4 else [0]
    return _moved(R, ordinary_batch(R, n_q, seed), sorted(set(rows)), 2.2, True)


def beyond_batch(R, n_q, seed=31):
    """beyond the headroom: an ordinary batch with one finite row at |x'|^2 = 7 M_ref"""
    return _moved(R, ordinary_batch(R, n_q, seed), [n_q // 2], 7.0, False)


def band(n_cols, R):
    """(S, e0, kappa) of the resident scale: test_wide_model --band with M_res = 4 M_ref as the device forms it"""
    m = HEADROOM * float(F32(m_ref(R) * (1.0 + 4e-7)))
    exe = os.path.join(ROOT, "clustering_amd", "bin", "test_wide_model")
    out = subprocess.run([exe, "--band", str(n_cols), repr(m)], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    assert out[0] == "band" and int(out[1]) == n_cols
    return float(out[2]), float(out[3]), float(out[4])


def realised_error_share(n_cols, R, radii):
    """An estimate of how far the accumulator of a pair near a threshold lies from S d2, as a share of the window's
    half-width eps -- from the number formats, not from the device.  The band eps is a sum of worst-case bounds; what
    realises is
      the chain's roundings: NM MFMAs, each truncating four addends and rounding once (4.5 u, u = 2^-24, the hardware model
        of guard_e0), relative to partial sums of at most S (|x| + |y|)^2 <= S M_res for rows within M_ref of the origin,
        signed, so they add up as sqrt(NM);
      the two fp16 pieces per coordinate: 2^-22 relative per factor, 2^-21 per product, on sum |x_k y_k| <= |x| |y| <= M_res / 4;
    over the smallest eps of the call's radii.  A pair can be parked by the device and not counted in float64, or the
    reverse, only if |d2 - r^2| lies within this share of the window's edge."""
    s, e0, kappa = band(n_cols, R)
    sm = s * HEADROOM * m_ref(R)
    nm = cw.nm_for(n_cols)
    err = 4.5 * 2.0 ** -24 * sm * np.sqrt(nm) + 2.0 ** -21 * sm / 4.0
    eps = min(e0 + kappa * s * float(F32(r) * F32(r)) for r in radii)
    return float(err / eps)


def window_pairs(n_cols, Q, R, perm_q, perm_r, radii, widen=1.0):
    """crosswidepruneref.exact_band_pairs under the resident band: pairs of the surviving block pairs with
    |d2 - r^2| < widen x eps at some radius, added over the radii, d2 in float64 -> (pairs in the window, surviving block pairs)"""
    g = pr.gaps(Q, R, perm_q, perm_r)
    near = g < 1.001 * max(pr.launch_r2max(radii))
    s, e0, kappa = band(n_cols, R)
    q64, r64 = Q[perm_q].astype(np.float64), R[perm_r].astype(np.float64)
    total = 0
    for r in radii:
        r2 = float(F32(r) * F32(r))
        e = widen * (e0 + kappa * s * r2) / s
        for qb in range(g.shape[0]):
            rows = np.flatnonzero(near[qb])
            if len(rows) == 0:
                continue
            ref = np.concatenate([r64[BLOCK * b:BLOCK * (b + 1)] for b in rows])
            qq = q64[BLOCK * qb:BLOCK * (qb + 1)]
            d2 = (qq * qq).sum(1)[:, None] + (ref * ref).sum(1)[None, :] - 2.0 * qq @ ref.T
            total += int((np.abs(d2 - r2) < e).sum())
    return total, int(near.sum())


# the references of the GPU module: (rows, columns); 1 500 rows are 12 blocks in one share, 8 320 x 80 are 65 blocks in several
REFERENCES = ((1500, 65), (1500, 100), (1500, 256), (8320, 80))
BATCHES = (300, 1, 129, 1100, 127, 128)   # interleaved: no size follows its neighbour in size
MAX_BATCH = 1100


def reference_rows(n_r, n_cols):
    return cw.blob_sets(n_cols, 8, n_r, seed=7)[1]


def prune_case():
    """the pruning case, (Q, R, fe_q, fe_r): crosswidennpruneref.split_case(1500, 1500, 65) -- stretched rows, queries and
    reference of one cloud, the free energies of their populations"""
    import crosswidennpruneref as nnref
    return nnref.split_case(1500, 1500, 65)
