"""GPU (-m gpu): the cross sweeps (dc_hip_*_cross_dev) at the edges the self sweeps are held to, against the probe's
canonical d2 (the [n_q, n_r] block of the union, tests/crossref.py) and never against another GPU variant: radii of 0,
1e-30, inf, 1e20 (fl32(r*r) = inf) and NaN, alone and mixed, repeated, more than one launch takes, unsorted straight
into the C ABI; ties exactly at the radius and pairs one float inside or outside it; degenerate data and data at the
clamps of the population scale, with Q and R chosen apart; the statistics flag in one set only; reference counts across
the 32-row tile; the free energies on another maximum; a seeded fuzz; and the avx / fma summation orders.

Every matrix-core call also reads header word 1 of the cross workspace afterwards: 0 where the matrix-core kernel was
meant to answer, non-zero where the case trips the statistics flag (the exact kernel answers)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fe_families
from crossref import (F32, bits, block_d2, expect_nn, expect_pops, fe_of, gpu, host, radius, same_nn, sets, square,
                      stats_flagged, variants)
from clustering_amd.synth import gaussian_blobs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def dens():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from clustering_amd import density
    return density


@pytest.fixture(scope="module")
def probe():
    from clustering_amd import capi
    from oracle.oracle import Probe
    return Probe(capi.CANON_ORDER)


def flag_word(dens, t):
    """header word 1 of the cross workspace on t's device: the statistics flag of the last cross sweep"""
    return int(dens._cross_workspace(t.device).buf[4:8].cpu().numpy().view(np.uint32)[0])


def answered(dens, q, v, flagged, what):
    """after a matrix-core call (n_cols <= 64): 0 in word 1 -- the matrix-core kernel answered -- unless the case trips
    the flag"""
    if v == "direct" or q.shape[1] > 64:
        return
    w = flag_word(dens, q)
    if flagged:
        assert w != 0, (what, "the statistics flag should be set")
    else:
        assert w == 0, (what, "the matrix-core kernel should have answered, flag word", w)


def pops_abi(dens, q, r, radii, variant, i_from=0, i_to=None):
    """dc_hip_populations_cross_dev called directly, radii in the caller's order (no sorting on the way)"""
    import torch
    from clustering_amd import capi
    n_q, D = q.shape
    n_r = r.shape[0]
    i_to = n_q if i_to is None else i_to
    rad = np.ascontiguousarray(radii, dtype=np.float32)
    out = torch.empty((rad.size, n_q), dtype=torch.int32, device=q.device)
    ws, ws_bytes = dens._cross_workspace(q.device).get(n_q, n_r, D)
    rc = capi.lib.dc_hip_populations_cross_dev(
        C.c_void_p(q.data_ptr()), n_q, C.c_void_p(r.data_ptr()), n_r, D, rad.ctypes.data_as(C.POINTER(C.c_float)),
        rad.size, i_from, i_to, C.c_void_p(out.data_ptr()), ws, ws_bytes, capi.VARIANTS[variant],
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    capi.check(rc, "dc_hip_populations_cross_dev")
    return out


def same_pops(got, want, what):
    g = host(got)
    if not (g == want).all():
        bad = np.argwhere(g != want)
        k, i = bad[0]
        pytest.fail(f"pops {what}: {len(bad)} entries differ, e.g. radius {k} query {i}: {g[k, i]} != {want[k, i]}")


class Case:
    """one (Q, R) pair on the device with its canonical d2 block"""

    def __init__(self, dens, probe, Q, R, flagged=False, what=""):
        self.Q = np.ascontiguousarray(Q, dtype=np.float32)
        self.R = np.ascontiguousarray(R, dtype=np.float32)
        self.what = what
        self.flagged = flagged
        assert stats_flagged(self.Q, self.R) == flagged, (what, "the case does not reach the path it is meant to")
        self.dens = dens
        self.d2 = block_d2(probe, self.Q, self.R)
        self.q, self.r = gpu(self.Q), gpu(self.R)
        self.D = self.Q.shape[1]

    def pops(self, radii, i_from=0, i_to=None, abi=False):
        """populations of every variant (through Python, or -- abi=True -- straight into the C ABI, radii unsorted)"""
        want = expect_pops(self.d2, radii, i_from, i_to)
        live = (i_to is None or i_from < i_to) and len(self.R) > 0
        for v in variants(self.D):
            what = (self.what, "radii", radii, "rows", i_from, i_to, v, "abi" if abi else "python")
            if abi:
                got = pops_abi(self.dens, self.q, self.r, radii, v, i_from, i_to)
            else:
                got = self.dens.calculate_populations_against(self.q, self.r, radii, i_from, i_to, variant=v)
            if live:
                answered(self.dens, self.q, v, self.flagged, what)
            same_pops(got, want, what)
        return want

    def nn(self, fe_q=None, fe_r=None, i_from=0, i_to=None):
        """nn / nn_hd with the given free energies (seeded normal draws if none) and nn only, every variant"""
        if fe_q is None:
            rng = np.random.default_rng(len(self.Q) + 3 * len(self.R))
            fe_q = rng.normal(size=len(self.Q)).astype(np.float32)
            fe_r = rng.normal(size=len(self.R)).astype(np.float32)
        exp = expect_nn(self.d2, fe_q, fe_r, i_from, i_to)
        live = (i_to is None or i_from < i_to) and len(self.R) > 0
        for v in variants(self.D):
            what = (self.what, "nn", i_from, i_to, v)
            got = self.dens.nearest_reference(self.q, self.r, gpu(fe_q), gpu(fe_r), i_from, i_to, variant=v)
            if live:
                answered(self.dens, self.q, v, self.flagged, what)
            same_nn(got, exp, what)
            got = self.dens.nearest_reference(self.q, self.r, i_from=i_from, i_to=i_to, variant=v)
            if live:
                answered(self.dens, self.q, v, self.flagged, what + ("nn only",))
            assert got[2] is None and got[3] is None
            same_nn(got, exp[:2], what + ("nn only",))
        return exp


# ---- radii ----------------------------------------------------------------------------------------------------------
def edge_radii(D):
    r0 = radius(D)
    return [[0.0], [1e-30], [INF], [1e20], [NAN], [r0, INF], [0.0, r0], [1e-30, 1e20, 0.75 * r0], [r0, NAN, INF],
            [NAN, r0], [r0, r0]]


@pytest.mark.parametrize("D", [3, 10, 30, 64])
def test_radius_edges(dens, probe, D):
    """r = 0 and 1e-30 (fl32(r*r) = 0: nothing inside, not even a copy), inf and 1e20 (every finite pair inside), NaN
    (nothing inside), alone and next to ordinary radii (the images of a launch are scaled for its largest r^2), a radius
    given twice, 9 and 17 radii in permuted order (more than kMaxRadiiPerLaunch: each chunk prepares the header again).
    The multi-radius and NaN cases also go straight into the C ABI unsorted."""
    Q, R = sets(D, 300, 700, seed=40 + D)
    c = Case(dens, probe, Q, R, what=f"D={D}")
    rng = np.random.default_rng(D)
    lists = edge_radii(D)
    for k in (9, 17):
        lists.append([float(x) for x in rng.permutation(np.linspace(0.1, 3.0, k).astype(np.float32) * radius(D))])
    for radii in lists:
        want = c.pops(radii)
        if len(radii) > 1 or np.isnan(radii).any():
            c.pops(radii, abi=True)
        assert (want[np.isnan(radii)] == 0).all()
        assert (want[[x in (INF, 1e20) for x in radii]] == len(R)).all()
    c.pops(lists[-1], 37, 250)
    c.pops(lists[-1], 37, 250, abi=True)
    c.nn()


@pytest.mark.parametrize("D", [3, 10, 30, 64])
def test_reference_counts_across_the_tile(dens, probe, D):
    """n_ref around the 32-row tile with an infinite radius: the pad rows of the last reference tile meet a threshold of
    -inf and must stay outside (norm +inf), so every query counts exactly n_ref"""
    for n_ref in (31, 32, 33, 63, 65):
        Q, R = sets(D, 100, n_ref, seed=n_ref + D)
        c = Case(dens, probe, Q, R, what=f"D={D} n_ref={n_ref}")
        for radii in ([INF], [radius(D), INF], [1e20]):
            want = c.pops(radii)
            assert (want[-1] == n_ref).all()
        c.pops([INF, radius(D), NAN], abi=True)
        c.nn()


# ---- ties at the radius -----------------------------------------------------------------------------------------------
def radii_at(T):
    """float radii near sqrt(T) with fl32(r*r) equal to T (pairs at T are outside: the comparison is a strict <), to the
    float above T (they are inside) and to the float below T -- those of the three that some float radius reaches"""
    T = F32(T)
    targets = (T, np.nextafter(T, F32(np.inf)), np.nextafter(T, F32(0.0)))
    base = np.array([np.sqrt(np.float64(T))], dtype=np.float32).view(np.uint32)[0]
    cands = (int(base) + np.arange(-16, 17, dtype=np.int64)).astype(np.uint32).view(np.float32)
    out = []
    for t in targets:
        hit = [float(r) for r in cands if square(r) == t]
        if hit:
            out.append(hit[0])
    return out


def lattice_sets(D, seed):
    """queries and references on a lattice of spacing 0.25, the queries offset from references by whole spacings in a
    few columns, the references with exact copies: d2 = 0.0625 m, exact in every summation order"""
    rng = np.random.default_rng(seed)
    R = (rng.integers(0, 4, (600, D)) * 0.25).astype(np.float32)
    R[rng.integers(0, 600, 150)] = R[rng.integers(0, 600, 150)]
    Q = R[rng.integers(0, 600, 280)].copy()
    step = rng.choice([-1, 0, 0, 0, 0, 0, 1], size=Q.shape) if D > 3 else rng.integers(-1, 2, size=Q.shape)
    Q = (Q + 0.25 * step).astype(np.float32)
    return Q, R


@pytest.mark.parametrize("D", [3, 10, 30, 64])
def test_ties_at_the_radius(dens, probe, D):
    """pairs exactly at the radius, one float inside and one float outside it -- all in the guard band of the Gram form,
    so only the canonical re-check decides them; many references at one d2 for the neighbours (lowest index wins)"""
    Q, R = lattice_sets(D, 70 + D)
    c = Case(dens, probe, Q, R, what=f"lattice D={D}")
    levels = np.unique(c.d2[c.d2 > 0])
    targets = list(levels[:5]) + list(levels[len(levels) // 3: len(levels) // 3 + 2])
    every = []
    for T in targets:
        radii = radii_at(T)
        if not radii:
            continue
        want = c.pops(radii)
        for k, r in enumerate(radii):   # the strict < at the tie: a radius whose square is T leaves the T-pairs out
            if square(r) == T:
                assert (want[k] == (c.d2 < T).sum(axis=1)).all()
        every += radii
    assert len(every) >= 6, every
    c.pops(every, abi=True)
    exp = c.nn()
    assert ((c.d2 == exp[1][:, None]).sum(axis=1) > 1).any()   # (references tied at the nearest d2)


# ---- scale and degenerate data ------------------------------------------------------------------------------------------
def degenerate_cases(D):
    rng = np.random.default_rng(80 + D)
    r0 = radius(D)
    base_q, base_r = sets(D, 400, 900, seed=90 + D)
    two_q = np.concatenate([np.zeros((150, D)), np.ones((150, D)) * 1e3])
    two_r = np.concatenate([np.ones((200, D)) * 1e3, np.zeros((300, D))])

    def const_col(n):
        return np.concatenate([rng.normal(size=(n, D - 2)), np.full((n, 1), 7.0), rng.normal(size=(n, 1)) * 1e6], 1)

    cases = [
        ("identical rows", np.full((400, D), 0.37), np.full((700, D), 0.37), [0.0, 1e-3, 1.0]),
        ("all zero", np.zeros((300, D)), np.zeros((500, D)), [0.5]),
        ("all zero, r = 0", np.zeros((300, D)), np.zeros((500, D)), [0.0]),
        ("one query row repeated", np.repeat(base_r[5:6], 300, axis=0), base_r, [r0, 2 * r0]),
        ("one reference row repeated", base_q, np.repeat(base_q[7:8] + F32(0.01), 500, axis=0), [r0, 2 * r0]),
        ("two far points, tiny radius", two_q, two_r, [1e-6, 10.0]),
        ("radius beyond everything", two_q, two_r, [1e9]),
        ("constant and huge column", const_col(400), const_col(700), [3.0, 1e6]),
        ("one query", base_q[:1], base_r, [r0, 2 * r0]),
        ("one reference", base_q, base_r[:1], [r0, 2 * r0, INF]),
    ]
    for s in (1e-17, 1e-15, 1e15, 3e17):
        cases.append((f"scale {s}", base_q * F32(s), base_r * F32(s), [r0 * s, 0.6 * r0 * s, 1e6 * s]))
    return cases


@pytest.mark.parametrize("D", [3, 10, 30, 64])
def test_scale_and_degenerate_data(dens, probe, D):
    """M = 0 (identical rows, all zero: every pair in the band), one set a single repeated row, far points with a tiny
    radius and a radius beyond everything, both sets at 1e-17 (beyond the upper clamp of pick_scale_pop), 1e-15, 1e15
    and 3e17 (|x'|^2 still below the 1e36 of the flag), a constant column next to a 1e6 column, one query, one
    reference -- every one of them answered by the matrix-core kernel"""
    for name, Q, R, radii in degenerate_cases(D):
        c = Case(dens, probe, Q, R, what=f"{name}, D={D}")
        c.pops(radii)
        c.nn()


@pytest.mark.parametrize("D", [3, 10, 64])
def test_overflow_flag_in_one_set(dens, probe, D):
    """a row whose |x - mean|^2 passes 1e36 in the queries only, then in the references only: the statistics pass of
    BOTH sets must see it, the flag is set and the exact kernel gives the probe's values"""
    r0 = radius(D)
    Q, R = sets(D, 300, 600, seed=150 + D)
    Qb = Q.copy()
    Qb[17, 0] = F32(2e18)
    c = Case(dens, probe, Qb, R, flagged=True, what=f"overflow in Q, D={D}")
    c.pops([r0, INF])
    c.nn()
    Rb = R.copy()
    Rb[400, D - 1] = F32(-2e18)
    c = Case(dens, probe, Q, Rb, flagged=True, what=f"overflow in R, D={D}")
    c.pops([r0, 2 * r0, INF])
    c.nn()
    # ... and the next call on clean data is answered by the matrix cores again
    Case(dens, probe, Q, R, what=f"clean after the flag, D={D}").pops([r0])


# ---- free energies on another scale -------------------------------------------------------------------------------------
def test_free_energies_against_another_maximum_at_the_float_edges(dens):
    """pops and maxima where (float)pop and 1.0f / max_pop round: 2^24 - 1, 2^24, 2^24 + 1, 2^31 - 1"""
    import torch
    pops = np.array([0, 1, 2, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 31 - 1], dtype=np.int32)
    for mx in (1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 1, 2 ** 32 - 1):
        got = host(dens.calculate_free_energies_against(torch.from_numpy(pops).cuda(), mx))
        assert (bits(got) == bits(fe_of(pops, mx))).all(), (mx, got, fe_of(pops, mx))


# ---- cross fuzz against the probe ---------------------------------------------------------------------------------------
SIZES = [1, 2, 31, 32, 33, 64, 257, 1000, 2500]


def fuzz_case(dens, probe, rng):
    """one random cross case; every output bit for bit against the probe, the parameters in every message"""
    while True:
        n_q, n_r = (int(x) for x in rng.choice(SIZES, 2))
        if n_q + n_r <= 4000:
            break
    u = rng.random()
    D = int(rng.integers(1, 65)) if u < 0.8 else (int(rng.integers(65, 121)) if u < 0.93 else int(rng.integers(401, 421)))
    kind = int(rng.integers(0, 6))
    sig = float(rng.choice([0.02, 0.08, 0.3]))
    c = gaussian_blobs(n_q + n_r, D, seed=int(rng.integers(1, 1 << 30)), sigma=sig)
    scale = sig * np.sqrt(D) + 0.5
    if kind == 4:   # clusters over the plane of columns 0 / 1, a few far outliers
        k = int(rng.choice([2, 5, 40]))
        spread = float(rng.choice([1.0, 30.0, 3000.0])) * sig * np.sqrt(D)
        cen = np.zeros((k, D))
        cen[:, :min(D, 2)] = rng.uniform(-spread, spread, size=(k, min(D, 2)))
        c = (cen[rng.integers(0, k, n_q + n_r)] + rng.normal(0.0, sig, size=(n_q + n_r, D))).astype(np.float32)
        c[rng.integers(0, n_q + n_r, max(1, (n_q + n_r) // 300))] += F32(50.0 * spread)
        scale = sig * np.sqrt(D)
    Q, R = c[:n_q].copy(), c[n_q:].copy()
    if kind == 1 or rng.random() < 0.3:   # duplicates within and across the sets
        R[rng.integers(0, n_r, max(1, n_r // 8))] = R[rng.integers(0, n_r, max(1, n_r // 8))]
        Q[rng.integers(0, n_q, max(1, n_q // 4))] = R[rng.integers(0, n_r, max(1, n_q // 4))]
    if kind == 2:   # the queries offset from the reference
        Q += F32(rng.choice([0.3, 10.0, 1e3, 1e4]))
    if kind == 3:   # both sets far from unit scale
        s = F32(10.0 ** rng.uniform(-12.0, 8.0))
        Q, R, scale = Q * s, R * s, scale * float(s)
    if kind == 5:   # a tiny reference and wide queries, or the other way round
        if rng.random() < 0.5:
            R *= F32(1e-3)
        else:
            Q *= F32(1e-3)
    nonfinite = bool(rng.random() < 0.15)
    if nonfinite:
        for X in (Q, R):
            if rng.random() < 0.6:
                X[rng.integers(0, len(X)), rng.integers(0, D)] = rng.choice([np.inf, -np.inf, np.nan])
    Q, R = np.ascontiguousarray(Q, dtype=np.float32), np.ascontiguousarray(R, dtype=np.float32)
    radii = [float(x) for x in scale * rng.uniform(0.05, 1.5, size=int(rng.integers(1, 18)))]
    lo = int(rng.integers(0, n_q))
    hi = int(rng.integers(lo, n_q + 1))
    if rng.random() < 0.4:
        lo, hi = 0, n_q
    family = str(rng.choice(sorted(fe_families.FAMILIES))) if rng.random() < 0.7 else None
    params = dict(n_q=n_q, n_ref=n_r, D=D, kind=kind, sigma=sig, nonfinite=nonfinite, radii=radii, rows=(lo, hi),
                  fe=family)
    full = probe.pairwise_d2(np.vstack([Q, R]))
    d2 = full[:n_q, n_q:]
    flagged = stats_flagged(Q, R)
    q, r = gpu(Q), gpu(R)
    live = lo < hi
    pops_exp = expect_pops(d2, radii, lo, hi)
    fe_q = fe_r = None
    if family:
        r2 = square(radii[0])
        with np.errstate(invalid="ignore"):
            pops_r = (full[n_q:, n_q:] < r2).sum(axis=1).astype(np.uint64)
            pops_q = (d2 < r2).sum(axis=1).astype(np.uint64)
        fe_q = fe_families.make(family, Q, pops_q, seed=1)
        fe_r = fe_families.make(family, R, pops_r, seed=2)
    nn_exp = expect_nn(d2, fe_q, fe_r, lo, hi)
    for v in variants(D):
        what = (v, params)
        got = dens.calculate_populations_against(q, r, radii, lo, hi, variant=v)
        if live:
            answered(dens, q, v, flagged, what)
        same_pops(got, pops_exp, what)
        if family:
            got = dens.nearest_reference(q, r, gpu(fe_q), gpu(fe_r), lo, hi, variant=v)
            if live:   # (a NaN reference free energy hands the call to the exact kernel as well)
                answered(dens, q, v, flagged or bool(np.isnan(fe_r).any()), what)
        else:
            got = dens.nearest_reference(q, r, i_from=lo, i_to=hi, variant=v)
            if live:
                answered(dens, q, v, flagged, what)
        same_nn(got, nn_exp, what)


@pytest.mark.parametrize("seed", [41, 42, 43])
def test_cross_fuzz_against_the_probe(dens, probe, seed):
    rng = np.random.default_rng(seed)
    for case in range(40):
        try:
            fuzz_case(dens, probe, rng)
        except AssertionError as e:
            pytest.fail(f"cross fuzz, seed {seed}, case {case}: {e}")


# ---- the other summation orders -----------------------------------------------------------------------------------------
CHILD = r"""
import ctypes as C
import os
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from clustering_amd import capi, density as dens
from oracle.oracle import Probe
from crossref import bits, block_d2, expect_nn, expect_pops, gpu, host, radius, same_nn, sets, square, variants
ORDER = sys.argv[2]
assert capi.lib.dc_hip_canon_order().decode() == ORDER, capi.lib.dc_hip_canon_order()
probe, probe_sse2 = Probe(ORDER), Probe("sse2")
differ = 0
p = lambda a: a.ctypes.data_as(C.c_void_p)
for D in (3, 8, 9, 10, 16, 30, 64, 70, 401, 1000):
    n_q, n_r = (333, 777) if D <= 70 else (150, 300)
    Q, R = sets(D, n_q, n_r, seed=500 + D)     # (exact duplicates between and within the sets)
    d2 = block_d2(probe, Q, R)
    other = block_d2(probe_sse2, Q, R)
    diff = np.argwhere(bits(d2) != bits(other))
    differ += len(diff)
    r0 = radius(D)
    radii = [r0, 0.5 * r0, 2.0 * r0]
    # radii right at d2 values this order rounds differently: only the canonical re-check in ORDER decides them
    for a, b in diff[:6]:
        t = max(d2[a, b], other[a, b])
        base = int(np.array([np.sqrt(np.float64(t))], dtype=np.float32).view(np.uint32)[0])
        for rr in (base + np.arange(-8, 9, dtype=np.int64)).astype(np.uint32).view(np.float32):
            if square(rr) == t:
                radii.append(float(rr))
                break
    rng = np.random.default_rng(D)
    fe_q = rng.normal(size=n_q).astype(np.float32)
    fe_r = rng.normal(size=n_r).astype(np.float32)
    q, r = gpu(Q), gpu(R)
    for lo, hi in ((0, n_q), (n_q // 5, n_q - n_q // 7)):
        pops_exp = expect_pops(d2, radii, lo, hi)
        nn_exp = expect_nn(d2, fe_q, fe_r, lo, hi)
        for v in variants(D):
            what = (ORDER, D, lo, hi, v)
            got = dens.calculate_populations_against(q, r, radii, lo, hi, variant=v)
            if v != "direct" and D <= 64:   # (the matrix-core kernel answered)
                assert int(dens._cross_workspace(q.device).buf[4:8].cpu().numpy().view(np.uint32)[0]) == 0, what
            assert (host(got) == pops_exp).all(), what + ("pops",)
            same_nn(dens.nearest_reference(q, r, gpu(fe_q), gpu(fe_r), lo, hi, variant=v), nn_exp, what)
            same_nn(dens.nearest_reference(q, r, i_from=lo, i_to=hi, variant=v), nn_exp[:2], what + ("nn only",))
    # the host-pointer entry points (auto variant, their own workspace and stream)
    rad = np.array(radii, np.float32)
    lo, hi = 7, n_q - 3
    pops = np.zeros((len(rad), n_q), np.uint32)
    capi.check(capi.lib.dc_hip_populations_cross(p(Q), n_q, p(R), n_r, D, p(rad), len(rad), lo, hi, 0, p(pops)))
    assert (pops == expect_pops(d2, radii, lo, hi)).all(), (ORDER, D, "host pops")
    out = [np.zeros(n_q, np.uint32), np.zeros(n_q, np.float32), np.zeros(n_q, np.uint32), np.zeros(n_q, np.float32)]
    capi.check(capi.lib.dc_hip_nearest_neighbors_cross(p(Q), n_q, p(R), n_r, D, p(fe_q), p(fe_r), lo, hi, 0,
                                                       *[p(a) for a in out]))
    exp = expect_nn(d2, fe_q, fe_r, lo, hi)
    for k in (0, 2):
        assert (out[k].astype(np.int64) == exp[k]).all(), (ORDER, D, "host nn idx", k)
        assert (bits(out[k + 1]) == bits(exp[k + 1])).all(), (ORDER, D, "host nn d2", k)
assert differ > 0, "the two orders never differ on these sets: the test would not tell them apart"
print("ok: the canonical d2 of the two orders differ in", differ, "pairs")
"""


@pytest.mark.parametrize("order", ["avx", "fma"])
def test_cross_sweeps_in_the_other_orders(order):
    """the cross sweeps of the avx / fma libraries against the probe of that order (one process binds one library):
    every variant, a row range, nn only, the host-pointer entry points, radii at the d2 values the order rounds apart"""
    if not os.path.exists(os.path.join(ROOT, "clustering_amd", "lib_" + order, "libdcdensity.so")):
        pytest.fail(f"clustering_amd/lib_{order}/libdcdensity.so is missing: __graft_entry__.build() makes it")
    env = dict(os.environ, DC_CANON_ORDER=order)
    env.pop("DC_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, order], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
