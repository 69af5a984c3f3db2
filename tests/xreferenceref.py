"""Cases of the resident reference's tests at 257..1024 columns (dc_hip_reference_xwide_*):
tests/test_reference_xwide_cases.py checks their premises on the CPU, tests/test_gpu_xwide_reference.py runs them on the
device.  Importing this module needs neither a GPU nor torch.

Everything is built from what exists: the resident form's order, means, norms and batches of referencewideref (origin,
scale and grid from the REFERENCE alone, M_res = 4 M_ref), and the data that prunes at these widths, its radii and the
counter bounds of xcrosswidepruneref.  What is new here is the tail outlier -- a row whose whole excess over M_res lies in
ONE column beyond the first 256, which a gate that reads four columns per lane would pass -- and the resident band of these
widths restated in numpy (xwideref's guard_e0 / guard_kappa with M_res in M's place)."""
import functools

import numpy as np

import crosswidepruneref as cp
import crosswideref as cw
import referencewideref as rw
import xcrosswidepruneref as xc
import xwideref
from referencewideref import HEADROOM, headroom_batch, beyond_batch, means, m_ref, norms2, ordinary_batch, outside_box, reference_order  # noqa: F401
from widepruneref import BLOCK, launch_r2max
from xcrosswidepruneref import radii_for, split_case, split_sets  # noqa: F401  (stretched data: columns 0 / 1 x 8)

F32 = np.float32
COLS = (257, 512, 1024)          # the widths of the module: the ends and the middle
GATE_COLS = (300, 1023)          # ... and where the gate's last slot is partly filled (300 = 4 x 64 + 44, 1023 = 15 x 64 + 63)
BATCHES = rw.BATCHES             # 300, 1, 129, 1 100, 127, 128
MAX_BATCH = rw.MAX_BATCH
GATE_MARGIN = 1.0 + 4.0e-7       # the gate compares fl32(|x - mean|^2) (1 + 4e-7) with M_res
TAIL_FACTOR = 5.0                # |x - mean|^2 of the tail outlier, in M_ref
# twice the worst |accumulator - S d2| / band that test_xwide_model measured at the width; the factor 2
# covers the last-bit run-to-run difference of the means (dc_mfma_wide_kernels.hpp)
F_EXACT = {257: 2 * 0.0154, 512: 2 * 0.0104, 1024: 2 * 0.0077}


@functools.lru_cache(maxsize=None)
def reference_rows(n_r, n_cols):
    return rw.reference_rows(n_r, n_cols)


def radii9(n_cols):
    """nine radii around the intra-blob distance of reference_rows: two launches"""
    return cw.radii_for(n_cols, 9)


def tail_outlier_batch(R, n_q, seed=31):
    """an ordinary batch with ONE row at mean + d e_k, k = the last column (>= 256), d^2 = TAIL_FACTOR M_ref: beyond M_res
    as a whole, exactly at the mean in columns 0..255 -> (Q, the row)"""
    Q = ordinary_batch(R, n_q, seed).copy()
    row, k = n_q // 2, R.shape[1] - 1
    assert k >= 256
    x = means(R).astype(np.float64)
    x[k] += np.sqrt(TAIL_FACTOR * m_ref(R))
    Q[row] = x.astype(F32)
    return np.ascontiguousarray(Q), row


def head_norms2(X, R, cols=256):
    """norms2 over the first `cols` columns alone: what a gate of four columns per lane would sum"""
    return ((X[:, :cols] - means(R)[:cols]).astype(F32).astype(np.float64) ** 2).sum(axis=1)


def m_res(R):
    """M_res as the device forms it: four times the float M_ref with the statistics pass's rounding margin"""
    return HEADROOM * float(F32(m_ref(R)) * F32(GATE_MARGIN))


def band(n_cols, R, m=None):
    """(S, e0, kappa) of the resident scale: guard_band(M, 0, D, sc) with M = M_res (m: another extent in its place)"""
    m = m_res(R) if m is None else m
    s = xwideref.pick_scale_nn(m)
    return s, xwideref.guard_e0(float(F32(m) * F32(s)), n_cols), xwideref.guard_kappa(n_cols)


def half_width(n_cols, R, r, m=None):
    """the window's half-width at radius r in units of d2: (e0 + kappa S r^2) / S"""
    s, e0, kappa = band(n_cols, R, m)
    return (e0 + kappa * s * float(F32(r) * F32(r))) / s


def window_counts(n_cols, Q, R, perm_q, perm_r, radii, widens, m=None):
    """float64 counts of the pairs with |d2 - r^2| < widen x half_width at some radius, added over the radii (one launch:
    at most 8), for every widen -> [(over the block pairs with gap^2 < r2max: surely evaluated, over those with
    gap^2 < 1.001 r2max: all that can be evaluated)]"""
    assert len(radii) <= 8
    perm_q, perm_r = np.asarray(perm_q, dtype=np.int64), np.asarray(perm_r, dtype=np.int64)
    g = cp.gaps(Q, R, perm_q, perm_r)
    r2max = max(launch_r2max(radii))
    d2 = xc.cross_d2(Q[perm_q], R[perm_r])
    expand = lambda mask: np.repeat(np.repeat(mask, BLOCK, axis=0), BLOCK, axis=1)[:len(perm_q), :len(perm_r)]
    sure, may = expand(g < r2max), expand(g < 1.001 * r2max)
    out = []
    for w in widens:
        a = b = 0
        for r in radii:
            near = np.abs(d2 - float(F32(r) * F32(r))) < w * half_width(n_cols, R, r, m)
            a, b = a + int((near & sure).sum()), b + int((near & may).sum())
        out.append((a, b))
    return out


def windows_apart(n_cols, R, radii, widen=2.0):
    """no pair lies in the windows of two radii: the windows, widened, do not meet"""
    edges = sorted((float(F32(r) * F32(r)) - widen * half_width(n_cols, R, r), float(F32(r) * F32(r)) + widen * half_width(n_cols, R, r))
                   for r in radii)
    return all(a[1] < b[0] for a, b in zip(edges, edges[1:]))
