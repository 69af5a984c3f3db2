"""Free energies of any origin, for the neighbour tests (tests/test_oracle.py, tests/test_gpu_free_energy_inputs.py).

Every other neighbour test derives its free energies from populations: few distinct values, all >= 0 with minimum
exactly -0.0, finite, highest where the data is sparse.  The library also takes free energies from the caller (the
reference's nearest_neighbors signature, dc_hip_nearest_neighbors*, dc_hip_session_set_free_energies, the CLI's -D),
and the nearest neighbour of lower free energy depends on them.  Each family is a seeded function of
(coords, pops, rng) that returns float32 [n]; ``pops`` is only read by the families in NEEDS_POPS.
"""
import numpy as np

import refmath

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def _distinct(v):
    """v with equal values moved apart by a few ulps (order kept): every value distinct"""
    v = np.asarray(v, dtype=np.float32).copy()
    o = np.argsort(v, kind="stable")
    s = v[o]
    if s.size > 1 and (np.diff(s) <= 0).any():
        for k in range(1, s.size):
            if s[k] <= s[k - 1]:
                s[k] = np.nextafter(s[k - 1], F32(np.inf))
        v[o] = s
    return v


def _from_bits(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


def fe_pops(coords, pops, rng):
    """control: the free energies of the populations (refmath.free_energies == oracle.free_energies bit for bit)"""
    return refmath.free_energies(pops)


def fe_continuous(coords, pops, rng):
    """normal draws, all distinct: many values per quantisation level, "mixed" tiles everywhere"""
    return _distinct(rng.normal(0.0, 1.0, len(coords)).astype(np.float32))


def fe_rounded7(coords, pops, rng):
    """the population free energies printed with %e and read back: what the CLI's -D hands in"""
    return np.array(["%e" % float(x) for x in refmath.free_energies(pops)], dtype=np.float64).astype(np.float32)


def fe_constant(coords, pops, rng):
    """all 0.0: no lower neighbour anywhere"""
    return np.zeros(len(coords), dtype=np.float32)


def fe_constant_3_5(coords, pops, rng):
    """all 3.5: no lower neighbour anywhere, and the floor is not 0"""
    return np.full(len(coords), 3.5, dtype=np.float32)


def fe_ties_ulp(coords, pops, rng):
    """1.0f + k ulp, k in 0..7: distinct values inside one quantisation level, and exact ties"""
    return _from_bits(np.uint32(0x3F800000) + rng.integers(0, 8, len(coords)).astype(np.uint32))


def fe_signed_zero(coords, pops, rng):
    """-0.0 and +0.0 (which compare equal: -0.0 is not lower than +0.0), a few -1 and +1"""
    n = len(coords)
    v = np.where(rng.random(n) < 0.5, F32(-0.0), F32(0.0)).astype(np.float32)
    pick = rng.random(n)
    v[pick < 0.04] = -1.0
    v[pick > 0.96] = 1.0
    return v


def fe_huge_span(coords, pops, rng):
    """magnitudes from 1e-5 up to 3e38 of either sign, and +-FLT_MAX: fe_hi - fe_lo overflows"""
    n = len(coords)
    v = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-5.0, 38.5, n)
    v = v.astype(np.float32)
    if n >= 4:
        v[rng.integers(0, n)] = FLT_MAX
        v[rng.integers(0, n)] = -FLT_MAX
    return v


def fe_subnormal(coords, pops, rng):
    """distinct magnitudes from 1.4e-45 (one denormal ulp) to about 1.5e-38, a quarter of them negative: the
    ordering must not flush them to zero"""
    n = len(coords)
    mag = _distinct(_from_bits(rng.integers(1, 0x00A00000, n).astype(np.uint32)))
    return np.where(rng.random(n) < 0.25, -mag, mag).astype(np.float32)


def fe_inf(coords, pops, rng):
    """continuous with about 3 % +inf and 3 % -inf: below a +inf query every finite frame is lower, below -inf none"""
    n = len(coords)
    v = fe_continuous(coords, pops, rng)
    pick = rng.random(n)
    v[pick < 0.03] = np.inf
    v[pick > 0.97] = -np.inf
    return v


def fe_gradient(coords, pops, rng):
    """coords[:, 0]: tiles wholly lower or wholly higher than a query, the lower neighbour on one side"""
    return np.ascontiguousarray(coords[:, 0], dtype=np.float32).copy()


def fe_gradient_neg(coords, pops, rng):
    """-coords[:, 0]: the same, the other way round"""
    return (-np.ascontiguousarray(coords[:, 0], dtype=np.float32)).astype(np.float32)


def fe_anti_density(coords, pops, rng):
    """-(population free energy): lower neighbours far away in the sparse regions, weak pruning"""
    return (-refmath.free_energies(pops)).astype(np.float32)


def cluster_a(coords):
    """cluster A of fe_per_cluster: the frames at or below the median of column 0 (of two clusters of equal size apart
    along column 0: the whole first cluster)"""
    x = np.asarray(coords, dtype=np.float32)[:, 0]
    return x <= np.median(x)


def fe_per_cluster(coords, pops, rng):
    """2.0 on cluster A (cluster_a), a few levels from 0 to 0.75 elsewhere: no frame of A is lower than another, so every
    frame of A has its lower neighbour in the other cluster"""
    a = cluster_a(coords)
    return np.where(a, F32(2.0), (0.25 * rng.integers(0, 4, len(coords))).astype(np.float32)).astype(np.float32)


def fe_nan(coords, pops, rng):
    """continuous with about 1 % NaN (at least one), of either sign: a NaN is never lower and has no lower neighbour"""
    n = len(coords)
    v = fe_continuous(coords, pops, rng)
    m = rng.random(n) < 0.01
    if n:
        m[rng.integers(0, n)] = True
    u = v.view(np.uint32)
    u[m] = np.where(rng.random(int(m.sum())) < 0.5, np.uint32(0x7FC00000), np.uint32(0xFFC00000))
    return v


FAMILIES = {
    "pops": fe_pops,
    "continuous": fe_continuous,
    "rounded7": fe_rounded7,
    "constant": fe_constant,
    "constant_3_5": fe_constant_3_5,
    "ties_ulp": fe_ties_ulp,
    "signed_zero": fe_signed_zero,
    "huge_span": fe_huge_span,
    "subnormal": fe_subnormal,
    "inf": fe_inf,
    "gradient": fe_gradient,
    "gradient_neg": fe_gradient_neg,
    "anti_density": fe_anti_density,
    "per_cluster": fe_per_cluster,
    "nan": fe_nan,
}
NEEDS_POPS = ("pops", "rounded7", "anti_density")


def make(name, coords, pops=None, seed=0):
    """family ``name`` on coords (pops: the populations of one radius, read by NEEDS_POPS only), seeded"""
    assert name in FAMILIES and (pops is not None or name not in NEEDS_POPS), name
    rng = np.random.default_rng([seed, sorted(FAMILIES).index(name), len(coords)])
    fe = FAMILIES[name](coords, pops, rng)
    assert fe.dtype == np.float32 and fe.shape == (len(coords),), name
    return np.ascontiguousarray(fe)
