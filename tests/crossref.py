"""Referees and plumbing of the cross-sweep tests (tests/test_gpu_cross.py, tests/test_gpu_cross_edges.py and the
child processes of the other summation orders): exact values from the probe's canonical d2 matrix, the reference's loop
shape, and nothing computed on the GPU.  Importing this module needs neither a GPU nor torch."""
import math

import numpy as np

from clustering_amd.synth import gaussian_blobs

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
NORM_LIMIT = F32(1.0e36)   # dc_mfma_kernels.hpp kNormLimit: a row with a larger |x - mean|^2 raises the statistics flag


def variants(D):
    return ("auto", "direct", "mfma") if D <= 64 else ("auto", "direct")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.cpu().numpy()


def block_d2(probe, Q, R):
    """canonical d2 of every (query, reference) pair: the [n_q, n_r] block of the probe's matrix of the union"""
    n_q = len(Q)
    return probe.pairwise_d2(np.vstack([Q, R]))[:n_q, n_q:]


def square(r):
    """fl32(r * r), as the library squares a radius (inf for |r| >= ~1.8e19, NaN for NaN)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return F32(r) * F32(r)


def expect_pops(d2, radii, i_from=0, i_to=None):
    i_to = d2.shape[0] if i_to is None else i_to
    out = np.zeros((len(radii), d2.shape[0]), dtype=np.int64)
    for k, r in enumerate(radii):
        r2 = square(r)
        with np.errstate(invalid="ignore"):
            out[k, i_from:i_to] = (d2[i_from:i_to] < r2).sum(axis=1)
    return out


def lexi_min(d2, allowed):
    """per row the lexicographic minimum of (d2, j) over allowed candidates with d2 < FLT_MAX -> (idx, d2)"""
    n_q, n_r = d2.shape
    with np.errstate(invalid="ignore"):
        ok = allowed & (d2 < FLT_MAX)
    v = np.where(ok, d2, np.inf)
    m = v.min(axis=1) if n_r else np.full(n_q, np.inf)
    has = np.isfinite(m)
    idx = np.where(has, np.argmax(ok & (v == m[:, None]), axis=1) if n_r else 0, n_r + 1).astype(np.int64)
    return idx, np.where(has, m, FLT_MAX).astype(np.float32)


def expect_nn(d2, fe_q=None, fe_r=None, i_from=0, i_to=None):
    n_q, n_r = d2.shape
    i_to = n_q if i_to is None else i_to
    nn_i, nn_d = lexi_min(d2, np.ones_like(d2, dtype=bool))
    out = [nn_i, nn_d]
    if fe_q is not None:
        with np.errstate(invalid="ignore"):
            out += list(lexi_min(d2, fe_r[None, :] < fe_q[:, None]))
    rows = np.zeros(n_q, dtype=bool)
    rows[i_from:i_to] = True
    for k in range(0, len(out), 2):
        out[k] = np.where(rows, out[k], n_r + 1)
        out[k + 1] = np.where(rows, out[k + 1], FLT_MAX).astype(np.float32)
    return out


def same_nn(got, exp, what):
    g = [host(t) for t in got if t is not None]
    assert len(g) == len(exp), what
    for k in range(0, len(exp), 2):
        assert (g[k].astype(np.int64) == exp[k]).all(), (what, "idx", k, np.flatnonzero(g[k] != exp[k])[:5])
        assert (bits(g[k + 1]) == bits(exp[k + 1])).all(), (what, "d2", k)


def sets(D, n_q, n_r, seed):
    """queries and references from the same blobs, with exact duplicates between and within the sets"""
    c = gaussian_blobs(n_q + n_r, D, seed=seed)
    rng = np.random.default_rng(seed)
    Q, R = c[:n_q].copy(), c[n_q:].copy()
    if n_q >= 8 and n_r >= 8:
        Q[rng.integers(0, n_q, n_q // 8)] = R[rng.integers(0, n_r, n_q // 8)]
        R[rng.integers(0, n_r, n_r // 16)] = R[rng.integers(0, n_r, n_r // 16)]
    return Q, R


def radius(D):
    return 0.2 if D <= 10 else float(0.08 * np.sqrt(2.0 * D))


def fe_of(pops, max_pop):
    """the free energies of the reference's formula, with the host libm"""
    rec = F32(1.0) / F32(max_pop)
    return np.array([F32(-math.log(float(F32(F32(p) * rec)))) if p else F32(np.inf) for p in pops], dtype=np.float32)


def stats_flagged(Q, R):
    """True where the statistics pass of a cross sweep (dc_mfma.hip cross_prepare: one mean over Q and R together,
    then rowstats_kernel over each set) flags the data: a non-finite row, or a row with fl32(|x - mean|^2) > 1e36 --
    the sweep then leaves the call to the exact kernel.  The same arithmetic: double column sums, the mean rounded to
    float (0 where it is not finite), x - mean in float, the squares summed in double and rounded once."""
    X = np.vstack([Q, R]).astype(np.float32)
    if X.shape[0] == 0:
        return False
    with np.errstate(over="ignore", invalid="ignore"):
        mu = (X.astype(np.float64).sum(axis=0) / X.shape[0]).astype(np.float32)
        mu = np.where(np.abs(mu) <= FLT_MAX, mu, F32(0.0)).astype(np.float32)
        v = (X - mu).astype(np.float32).astype(np.float64)
        nrm = (v * v).sum(axis=1).astype(np.float32)
        return bool((~(nrm <= NORM_LIMIT)).any())
