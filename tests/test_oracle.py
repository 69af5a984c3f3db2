"""CPU tests of the oracle itself (no GPU): KATs, the fast-math probe, an independent
numpy emulation, box-grid == brute force, and the reference-run statistics that
BASELINE.md section 2 records for the seeded generator."""
import json
import os

import numpy as np
import pytest

import fe_families
import refmath
from clustering_amd.synth import gaussian_blobs

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = json.load(open(os.path.join(HERE, "golden", "kat_cases.json")))["cases"]
FLT_MAX = np.finfo(np.float32).max


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_kat(oracle, case):
    c = np.array(case["coords"], dtype=np.float32)
    n = c.shape[0]
    radii = case["radii"]
    for boxgrid in (False, True):
        pops = oracle.populations(c, radii, boxgrid=boxgrid)
        assert pops.tolist() == case["pops"], (case["name"], boxgrid)
    sel = radii.index(case["fe_from_radius"])
    fe = oracle.free_energies(pops[sel])
    nn_idx, nn_d2, hd_idx, hd_d2 = oracle.nearest_neighbors(c, fe)
    assert nn_idx.tolist() == case["nn_idx"]
    assert hd_idx.tolist() == case["hd_idx"]
    assert (bits(nn_d2) == bits(np.array(case["nn_d2"], dtype=np.float32))).all()
    assert (bits(hd_d2) == bits(np.array(case["hd_d2"], dtype=np.float32))).all()
    # max-pop frame has fe == -0.0f
    assert bits(fe)[int(np.argmax(pops[sel]))] == 0x80000000
    assert n + 1 not in nn_idx.tolist() or n == 1


@pytest.mark.parametrize("D", list(range(1, 33)) + [40, 64])
def test_dist2_is_gcc_fastmath_order(oracle, probe, D):
    """canonical order == what g++ -O3 -ffast-math (reference flags) gives the reference's loop shape."""
    rng = np.random.default_rng(100 + D)
    c = rng.normal(0, 1, (48, D)).astype(np.float32)
    got = probe.pairwise_d2(c)
    want = refmath.d2_matrix(c)
    np.fill_diagonal(want, 0.0)
    assert (bits(got) == bits(want)).all()
    for i, j in [(0, 1), (5, 40), (47, 3)]:
        assert bits(oracle.dist2(c[i], c[j])) == bits(want[i, j])
        assert bits(oracle.dist2(c[j], c[i])) == bits(want[i, j])  # bitwise symmetric


def _fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, in exact rational arithmetic (round to nearest, ties to even; finite values)"""
    from fractions import Fraction
    v = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if v == 0:
        return np.float32(0.0)
    e = max(int(np.floor(np.log2(float(abs(v))))), -126)
    while abs(v) >= Fraction(2) ** (e + 1):
        e += 1
    while e > -126 and abs(v) < Fraction(2) ** e:
        e -= 1
    q = Fraction(2) ** (e - 23)
    n = v / q
    lo = n.numerator // n.denominator
    r = n - lo
    n_int = lo + (1 if (r > Fraction(1, 2) or (r == Fraction(1, 2) and lo % 2 == 1)) else 0)
    return np.float32(float(n_int * q))


def _avx_order_d2(x, y, fma=False):
    """numpy restatement of the AVX order (independent of dc_oracle.c): eight lane sums, b_i = a_i + a_{i+4}, (b0 + b2) +
    (b1 + b3); a four-column step (q0 + q2) + (q1 + q3); up to three scalar additions.  fma: the lane sums and the scalar
    tail with fused multiply-adds (one rounding), the four-column step unfused -- a -march=native build on AVX2 + FMA"""
    f = np.float32
    c = [f(a - b) for a, b in zip(x, y)]
    p = [f(v * v) for v in c]
    acc = (lambda a, k: _fma32(c[k], c[k], a)) if fma else (lambda a, k: f(a + p[k]))
    D, s, k = len(p), f(0.0), 0
    if D >= 8:
        a = [f(0.0)] * 8
        for k0 in range(0, 8 * (D // 8), 8):
            a = [acc(a[l], k0 + l) for l in range(8)]
        b = [f(a[i] + a[i + 4]) for i in range(4)]
        s, k = f(f(b[0] + b[2]) + f(b[1] + b[3])), 8 * (D // 8)
    if D - k >= 4:
        s, k = f(s + f(f(p[k] + p[k + 2]) + f(p[k + 1] + p[k + 3]))), k + 4
    for kk in range(k, D):
        s = acc(s, kk)
    return s


@pytest.mark.parametrize("order", ["avx", "fma"])
@pytest.mark.parametrize("D", list(range(1, 33)) + [40, 63, 64, 65])
def test_dist2_avx_order_is_gcc_fastmath_avx_order(D, order):
    """The summation orders of a reference built with -DCPU_ACCELERATION=AVX (CMakeLists.txt:73-76) or with
    -DNATIVE_COMPILATION on an AVX2 + FMA host (:53-56), which the library reproduces when built with `make CANON=avx` /
    `make CANON=fma`: oracle (order=...) == what g++ -O3 -ffast-math -mavx / -mavx2 -mfma gives the reference's loop shape
    == an independent numpy restatement, bit for bit."""
    from oracle.oracle import Oracle, Probe
    if order == "fma" and not all(f in open("/proc/cpuinfo").read() for f in (" avx2", " fma")):
        pytest.skip("this host has no AVX2 + FMA: the probe of that order cannot run here")
    o, pr = Oracle(order=order), Probe(order=order)
    rng = np.random.default_rng(300 + D)
    c = (rng.normal(0, 1, (40, D)) * rng.choice([1e-3, 1.0, 50.0])).astype(np.float32)
    got = pr.pairwise_d2(c)
    for i, j in [(0, 1), (5, 33), (39, 3), (7, 8), (20, 21)]:
        want = _avx_order_d2(c[i], c[j], fma=order == "fma")
        assert bits(got[i, j]) == bits(want) == bits(got[j, i])
        assert bits(o.dist2(c[i], c[j])) == bits(want) and bits(o.dist2(c[j], c[i])) == bits(want)
    full = np.array([[o.dist2(c[i], c[j]) if i != j else 0.0 for j in range(40)] for i in range(40)], dtype=np.float32)
    assert (bits(full) == bits(got)).all()


def test_fma_order_is_not_the_avx_order():
    """the fused lane sums round differently: the third build is not a copy of the second"""
    from oracle.oracle import Oracle
    rng = np.random.default_rng(9)
    c = rng.normal(0, 1, (64, 30)).astype(np.float32)
    a, b = Oracle(order="avx"), Oracle(order="fma")
    assert any(bits(a.dist2(c[0], c[j])) != bits(b.dist2(c[0], c[j])) for j in range(1, 64))


def test_avx_and_default_orders_differ_only_in_rounding():
    """the two orders are different roundings of the same sum: populations near a radius may differ by a frame or two"""
    from oracle.oracle import Oracle
    c = gaussian_blobs(3000, 10, seed=5)
    a = Oracle().populations(c, [0.2])
    for order in ("avx", "fma"):
        b = Oracle(order=order).populations(c, [0.2])
        assert abs(a.astype(np.int64) - b.astype(np.int64)).max() <= 2 and a.sum() > 0


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 7, 10, 12, 30])
def test_oracle_vs_numpy_emulation(oracle, D):
    c = gaussian_blobs(700, D, seed=7 + D)
    radii = [0.1, 0.25, 0.6] if D <= 10 else [0.5, 0.65, 0.9]
    want = refmath.populations(c, radii)
    assert (oracle.populations(c, radii) == want).all()
    assert (oracle.populations(c, radii, boxgrid=True) == want).all()
    fe = oracle.free_energies(want[1])
    assert (bits(fe) == bits(refmath.free_energies(want[1]))).all()
    got = oracle.nearest_neighbors(c, fe)
    exp = refmath.nearest_neighbors(c, fe)
    assert (got[0] == exp[0]).all() and (got[2] == exp[2]).all()
    assert (bits(got[1]) == bits(exp[1])).all() and (bits(got[3]) == bits(exp[3])).all()


def test_fe_matches_fastmath_probe(oracle, probe):
    rng = np.random.default_rng(3)
    for max_pop in (5, 314, 65950, 10**6, 2**24):
        pops = rng.integers(1, max_pop + 1, 20000).astype(np.uint64)
        pops[17] = max_pop
        assert (bits(oracle.free_energies(pops)) == bits(probe.free_energies(pops))).all()


def test_fe_strictly_monotone_in_pop(oracle):
    """fe[j] < fe[i]  <=>  pop[j] > pop[i]  (no float ties) up to 65950 and 10^6."""
    for max_pop in (65950, 10**6):
        pops = np.arange(1, max_pop + 1, dtype=np.uint64)
        fe = oracle.free_energies(pops)
        assert (np.diff(fe.astype(np.float64)) < 0).all()


def test_partial_rows_and_empty(oracle):
    c = gaussian_blobs(500, 5, seed=11)
    full = oracle.populations(c, [0.1, 0.2])
    a = oracle.populations(c, [0.1, 0.2], 0, 123)
    b = oracle.populations(c, [0.1, 0.2], 123, 500)
    assert (a[:, 123:] == 0).all() and (b[:, :123] == 0).all()
    assert (a + b == full).all()   # the host merge of cuda.cu:171-180 is a sum
    assert oracle.populations(np.zeros((0, 3), np.float32), [0.1]).shape == (1, 0)
    one = oracle.nearest_neighbors(np.zeros((1, 3), np.float32), np.zeros(1, np.float32))
    assert one[0][0] == 2 and one[1][0] == FLT_MAX


def test_reference_run_statistics_c1(oracle):
    """BASELINE.md section 2 (reference's own run, seed 20240): C1 r=0.1 mean pop 73.6, max 314."""
    c = gaussian_blobs(10000, 5)
    pops = oracle.populations(c, [0.1], boxgrid=True)[0]
    assert pops.max() == 314
    assert round(float(pops.mean()), 1) == 73.6


def test_reference_run_statistics_c2_subsample(oracle):
    """C2 (100k x 10) is too slow for the CPU suite in full; the 20k prefix of the same seeded
    stream pins the generator + oracle to fixed integers (regression pin, self-generated)."""
    c = gaussian_blobs(100000, 10)[:20000]
    pops = oracle.populations(c, [0.1, 0.2, 0.3], boxgrid=True)
    brute_rows = oracle.populations(c, [0.1, 0.2, 0.3], 0, 256)
    assert (pops[:, :256] == brute_rows[:, :256]).all()
    assert pops.shape == (3, 20000)
    assert (pops[0] <= pops[1]).all() and (pops[1] <= pops[2]).all()


def test_reference_run_statistics_c2(oracle):
    """BASELINE.md section 2 (reference's own run): C2 100k x 10, radii {0.1,0.2,0.3}: mean pops 2.8 / 719 / 9 223."""
    c = gaussian_blobs(100000, 10)
    pops = oracle.populations(c, [0.1, 0.2, 0.3], boxgrid=True)
    means = pops.mean(axis=1)
    assert round(float(means[0]), 1) == 2.8
    assert round(float(means[1])) == 719
    assert round(float(means[2])) == 9223


def test_screening_restatement_known_answers(oracle):
    """Hand-derived screening cases for oracle/screening_oracle.cpp (the reference ships no fixtures).
    Six frames on a line: {0, 0.1, 0.2}, {5, 5.1}, {9}; r = 0.15 gives pops 2 3 2 2 2 1, so frame 1 has
    the lowest free energy, frames 0 2 3 4 share ln(3/2) and frame 5 has ln 3.  sigma2 = mean nn d2 =
    (5 * 0.01 + 15.21) / 6, lumping distance 4 sigma2 = 10.17: 0-1-2 are mutual partners, 3-4 are, the two
    groups are 23 apart, frame 5 is alone."""
    from oracle.oracle import ScreeningOracle
    so = ScreeningOracle()
    c = np.array([[0.0], [0.1], [0.2], [5.0], [5.1], [9.0]], dtype=np.float32)
    pops = oracle.populations(c, [0.15])[0]
    assert list(pops) == [2, 3, 2, 2, 2, 1]
    fe = oracle.free_energies(pops)
    nn = oracle.nearest_neighbors(c, fe)
    # below 0.3 only frame 1; below 0.5 everything but frame 5; states numbered in order of first (lowest
    # free energy) member, unassigned frames 0
    assert list(so.screening(fe, nn[1], 0.3, c)) == [0, 1, 0, 0, 0, 0]
    first = so.screening(fe, nn[1], 0.5, c)
    assert list(first) == [1, 1, 1, 2, 2, 0]
    assert list(so.screening(fe, nn[1], 1.2, c, first)) == [1, 1, 1, 2, 2, 3]
    # microstates: frame 5 joins the state of its nearest lower-free-energy neighbour (frame 4);
    # renaming by population: the largest state gets the highest number... (sorted ascending, name = K - i)
    micro = so.assign_low_density(first, nn[2], fe)
    assert list(micro) == [1, 1, 1, 2, 2, 2]
    assert list(so.sorted_names(np.array([7, 7, 7, 3, 3, 9], dtype=np.uint64))) == [1, 1, 1, 2, 2, 3]


@pytest.mark.parametrize("family", sorted(fe_families.FAMILIES))
@pytest.mark.parametrize("n_rows,D", [(300, 3), (257, 10), (64, 30), (33, 2), (2, 5), (1, 4)])
def test_oracle_vs_numpy_emulation_free_energies_of_any_origin(oracle, family, n_rows, D):
    """The referee of tests/test_gpu_free_energy_inputs.py on exactly its inputs: free energies that do not come from
    populations (tests/fe_families.py: continuous, ties one ulp apart, +-0, spans that overflow, subnormals, +-inf,
    NaN, ...).  fe[j] < fe[i] is an IEEE comparison in both: NaN is never lower and a NaN frame has no lower neighbour,
    -0.0 is not lower than +0.0.  Indices equal, d2 bit-equal."""
    c = gaussian_blobs(n_rows, D, seed=900 + n_rows + D)
    if n_rows >= 64:
        c[5] = c[17]                 # an exact tie in d2
    pops = refmath.populations(c, [0.2 if D <= 10 else 0.08 * np.sqrt(2.0 * D)])[0]
    fe = fe_families.make(family, c, pops, seed=D)
    got = oracle.nearest_neighbors(c, fe)
    exp = refmath.nearest_neighbors(c, fe)
    assert (got[0] == exp[0]).all() and (got[2] == exp[2]).all()
    assert (bits(got[1]) == bits(exp[1])).all() and (bits(got[3]) == bits(exp[3])).all()
    if family == "nan":
        assert (got[2][np.isnan(fe)] == n_rows + 1).all() and (bits(got[3][np.isnan(fe)]) == bits(FLT_MAX)).all()
        assert not np.isnan(fe[got[2][got[2] <= n_rows].astype(np.int64)]).any()
    if family in ("constant", "constant_3_5"):
        assert (got[2] == n_rows + 1).all()
    if family == "signed_zero":
        hd = got[2] <= n_rows
        assert (fe[got[2][hd].astype(np.int64)] < fe[hd]).all()   # (a -0.0 frame is never the lower neighbour of +0.0)
