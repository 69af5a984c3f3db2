"""GPU tests of DC_VARIANT_MFMA32 (dc_mfma32.hpp), the fp32-input MFMA instance for n_cols 9 .. 10, at its edges: data
far from unit scale (the population image's scale c of scale32_pop at both of its clamps), radii of 0, 1e-30, inf and
radii whose fp32 square overflows, exact ties at the strict `<`, more radii than one launch takes, degenerate data,
rows the device gate hands to the direct kernels, ragged sizes and row ranges, the statistics flag, the refusals, and a
bounded seeded fuzz against the direct kernels.  Every oracle comparison holds check_full's standard: populations
bit-exact, free-energy bits, nn / nn_hd indices and d2 bits, sigma^2."""
import os
import subprocess
import sys

import numpy as np
import pytest

from clustering_amd.synth import gaussian_blobs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = np.finfo(np.float32).max
DIMS = [9, 10]
V = "mfma32"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def u64(t):
    return t.cpu().numpy().astype(np.uint32).astype(np.uint64)


@pytest.fixture(scope="module")
def dens():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from clustering_amd import density
    return density


def check_full(dens, oracle, c, radii, fe_from=0, what=""):
    """populations of every radius, the free energies of radius fe_from, nn / nn_hd and sigma^2 of mfma32 = oracle"""
    import torch
    c = np.ascontiguousarray(c, dtype=np.float32)
    ct = torch.from_numpy(c).cuda()
    pops = dens.calculate_populations_partial(ct, radii, variant=V)
    want = oracle.populations(c, radii)
    got = u64(pops)
    if not (got == want).all():
        bad = np.argwhere(got != want)[:4].tolist()
        pytest.fail(f"pops mismatch {what} radii={radii}: {len(np.argwhere(got != want))} entries, e.g. "
                    f"{[(r, i, int(got[r, i]), int(want[r, i])) for r, i in bad]}")
    fe = dens.calculate_free_energies(pops[fe_from].contiguous())
    fe_want = oracle.free_energies(want[fe_from])
    assert (bits(fe.cpu().numpy()) == bits(fe_want)).all(), f"fe bits {what}"
    nn = dens.nearest_neighbors_partial(ct, fe, variant=V)
    exp = oracle.nearest_neighbors(c, fe_want)
    g = [t.cpu().numpy() for t in nn]
    assert (g[0].astype(np.uint32).astype(np.uint64) == exp[0]).all(), f"nn idx {what}"
    assert (g[2].astype(np.uint32).astype(np.uint64) == exp[2]).all(), f"hd idx {what}"
    assert (bits(g[1]) == bits(exp[1])).all(), f"nn d2 bits {what}"
    assert (bits(g[3]) == bits(exp[3])).all(), f"hd d2 bits {what}"
    assert dens.compute_sigma2(nn[1]) == oracle.sigma2(exp[1]), f"sigma2 {what}"


def scale32_pop(M, r2max, D, K=10):
    """dc_mfma32.hpp scale32_pop in float64, WITHOUT its clamps: the scale c of the population image"""
    u = 2.0 ** -24
    eps1 = 1.25 * u * ((4.0 * K + 13.0) * M + (0.25 * D + 18.0) * max(r2max, 0.0))
    return np.sqrt((1.0 - 1.0 / 65536.0) / eps1) * (1.0 - 1.0 / 1048576.0) if eps1 > 1e-76 else np.inf


def max_centred_norm(c):
    x = c.astype(np.float64)
    return float(((x - x.mean(axis=0)) ** 2).sum(axis=1).max())


# ---- data far from unit scale ------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("scale", [1e-17, 1e-16, 1e-12, 1e-6, 1e4, 1e8, 3e17])
def test_scale_sweep(dens, oracle, scale, D):
    """test_data_far_from_unit_scale for mfma32: radii scale with the data.  At 1e-17 the unclamped c of scale32_pop is
    ~3.8e19, beyond its upper clamp (at 1e-16 it is ~3.8e18, inside); at 3e17 |x'|^2 stays below the 1e36 of the device
    gate, so the fp32 sweep itself answers, and the radius 1e6 s has an fp32 square of +inf."""
    base = gaussian_blobs(1300, D, seed=50 + D)
    c = (base * np.float32(scale)).astype(np.float32)
    r = float(np.sqrt(D) * 0.08 * 1.1)
    r2 = float(np.float32(r * scale) * np.float32(r * scale))
    c_free = scale32_pop(max_centred_norm(c), r2, D)
    if scale == 1e-17:
        assert c_free > 2.0 ** 64, c_free     # the case reaches the clamp: keep it that way
    if scale == 1e-16:
        assert c_free < 2.0 ** 63, c_free     # ... and its neighbour does not
    check_full(dens, oracle, c, [r * scale, 0.6 * r * scale], what=f"scale {scale}")
    check_full(dens, oracle, c, [1e6 * scale, 1e-9 * scale], what=f"scale {scale}, far radii")


# ---- radii -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", DIMS)
def test_radius_edges(dens, oracle, D):
    """r = 0 and 1e-30 (fl32(r*r) = 0), r = inf and 1e20 (fl32(r*r) = inf: every finite pair inside), r = NaN (no pair
    inside, not even the self pair: every population 1), with those radii alone and next to ordinary ones (one image per
    launch, scaled for the launch's largest r2); a radius given twice; 9 and 17 unsorted radii (more than
    kMaxRadiiPerLaunch: every launch chunk scales its image for its own r2max)"""
    c = gaussian_blobs(1500, D, seed=60 + D)
    nan, inf = float("nan"), float("inf")
    for radii in ([0.0], [1e-30], [inf], [1e20], [0.2, inf], [0.0, 0.2], [1e-30, 1e20, 0.15], [0.2, 0.2],
                  [nan], [nan, 0.2], [0.2, nan, inf]):
        check_full(dens, oracle, c, radii, what=f"radii {radii}")
    rng = np.random.default_rng(D)
    for k in (9, 17):
        radii = [float(x) for x in rng.permutation(np.linspace(0.02, 0.6, k).astype(np.float32))]
        check_full(dens, oracle, c, radii, fe_from=k // 2, what=f"{k} radii")


@pytest.mark.parametrize("D", DIMS)
def test_lattice_ties_at_the_radius(dens, oracle, D):
    """points on a lattice of spacing 0.25 with radii equal to 1, 2 and sqrt(2) spacings: pairs exactly at the radius,
    outside by the strict `<` -- all of them in the band of the Gram form"""
    rng = np.random.default_rng(70 + D)
    lattice = (rng.integers(0, 4, (1200, D)) * 0.25).astype(np.float32)
    check_full(dens, oracle, lattice, [0.25, 0.5, 0.3535534], what="lattice")
    check_full(dens, oracle, lattice, [0.25], what="lattice, one spacing alone")


# ---- degenerate data ---------------------------------------------------------------------------------------------

def degenerate_cases(D):
    rng = np.random.default_rng(80 + D)
    n = 3000
    two = np.concatenate([np.zeros((n // 2, D)), np.ones((n - n // 2, D)) * 1e3])
    base = gaussian_blobs(1400, D, seed=90 + D)
    dup = np.concatenate([base, base[:600], base[100:200]])
    dup = dup[rng.permutation(dup.shape[0])]
    return [
        ("identical rows", np.full((n, D), 0.37), [0.0, 1e-3, 1.0]),
        ("identical rows, r = 0 alone", np.full((n, D), 0.37), [0.0]),
        ("identical rows of 0.5, r = 0 alone", np.full((n, D), 0.5), [0.0]),
        ("all zero", np.zeros((n, D)), [0.5]),
        ("all zero, r = 0 alone", np.zeros((n, D)), [0.0]),
        ("two far points, tiny radius", two, [1e-6, 10.0]),
        ("radius beyond everything", two, [1e9]),
        ("constant and huge column", np.concatenate([rng.normal(size=(n, D - 2)), np.full((n, 1), 7.0),
                                                     rng.normal(size=(n, 1)) * 1e6], 1), [3.0, 1e6]),
        ("duplicated frames", dup, [0.2, 0.25]),
        ("offset +37.5", gaussian_blobs(1500, D, seed=100 + D) + np.float32(37.5), [0.2]),
        ("offset +1e4, sigma 0.02", gaussian_blobs(1500, D, seed=110 + D, sigma=0.02) + np.float32(1e4),
         [0.02 * np.sqrt(D), 0.01 * np.sqrt(D)]),
    ]


@pytest.mark.parametrize("D", DIMS)
def test_degenerate_inputs_against_the_oracle(dens, oracle, D):
    """test_degenerate_inputs_pruned_equals_direct for mfma32, against the oracle: M = 0 (identical rows, all zero),
    far pairs, a constant and a huge column, duplicates (lowest index wins), offsets (cancellation in the fp32 Gram form;
    the neighbour band is relative and unscaled)"""
    for name, c, radii in degenerate_cases(D):
        check_full(dens, oracle, c, radii, what=name)


@pytest.mark.parametrize("D", DIMS)
def test_gated_rows(dens, oracle, D):
    """rows with inf / -inf / NaN and data whose |x|^2 overflows: the device gate (hdr[1]) at the top of both mfma32
    kernels hands them to the direct kernels -- populations and neighbours"""
    c = gaussian_blobs(900, D, seed=120 + D)
    c[17, 3] = np.inf
    c[400, 0] = np.nan
    c[401, D - 1] = -np.inf
    check_full(dens, oracle, c, [0.2, 0.3], what="non-finite rows")
    huge = (gaussian_blobs(600, D, seed=130 + D) * np.float32(1e19)).astype(np.float32)
    check_full(dens, oracle, huge, [2e18], what="1e19")


# ---- sizes and row ranges ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", DIMS)
def test_ragged_sizes(dens, oracle, D):
    """sizes across the 32-row tile, the clump of 4 tiles, the 8 query tiles of a wave, the 8-tile norm batch and the
    chunking of the reference tiles over gridDim.y"""
    for n in (1, 2, 31, 32, 33, 127, 128, 129, 255, 256, 257, 1023, 1025, 4097):
        check_full(dens, oracle, gaussian_blobs(n, D, seed=140 + n), [0.2, 0.3], what=f"n={n}")


@pytest.mark.parametrize("D", DIMS)
def test_row_ranges(dens, oracle, D):
    """rows [lo, hi): populations 0 and neighbours "none" (index n + 1, d2 FLT_MAX) outside, the oracle's inside; the
    small ranges leave most waves idle (any_live == 0)"""
    import torch
    n = 1500
    c = gaussian_blobs(n, D, seed=150 + D)
    ct = torch.from_numpy(c).cuda()
    radii = [0.2, 0.3]
    full = oracle.populations(c, radii)
    fe = oracle.free_energies(full[0])
    fet = torch.from_numpy(fe).cuda()
    for lo, hi in ((0, 0), (0, 1), (n - 1, n), (5, 70), (33, 1000), (700, 702), (1, n - 1), (0, n)):
        p = u64(dens.calculate_populations_partial(ct, radii, lo, hi, variant=V))
        assert (p[:, :lo] == 0).all() and (p[:, hi:] == 0).all(), (lo, hi)
        assert (p[:, lo:hi] == full[:, lo:hi]).all(), (lo, hi)
        assert (p == oracle.populations(c, radii, lo, hi)).all(), (lo, hi)
        g = [t.cpu().numpy() for t in dens.nearest_neighbors_partial(ct, fet, lo, hi, variant=V)]
        exp = oracle.nearest_neighbors(c, fe, lo, hi)
        for k in (0, 2):
            idx = g[k].astype(np.uint32).astype(np.uint64)
            assert (idx == exp[k]).all(), (lo, hi, k)
            assert (idx[:lo] == n + 1).all() and (idx[hi:] == n + 1).all(), (lo, hi, k)
        for k in (1, 3):
            assert (bits(g[k]) == bits(exp[k])).all(), (lo, hi, k)
            assert (g[k][:lo] == FLT_MAX).all() and (g[k][hi:] == FLT_MAX).all(), (lo, hi, k)


# ---- the statistics flag -----------------------------------------------------------------------------------------

def test_stats_valid_flag_is_checked_on_the_device(dens, oracle):
    """DC_FLAG_STATS_VALID with mfma32: the neighbour call of a populations -> neighbours pair over ONE array gives the
    oracle's bits; claimed for another array of the same shape (or the same buffer rewritten in place) the device check
    flags the sweep and the direct kernels give the same bits"""
    import torch
    n, d = 4000, 10
    c1 = gaussian_blobs(n, d, seed=41)
    c2 = (gaussian_blobs(n, d, seed=42) * 37.0 + 5.0).astype(np.float32)     # other scale: stale statistics would hurt
    t1, t2 = torch.from_numpy(c1).cuda(), torch.from_numpy(c2).cuda()

    def reference(c, r):
        pops = oracle.populations(c, [r])
        fe = oracle.free_energies(pops[0])
        return pops, fe, oracle.nearest_neighbors(c, fe)

    def same(nn, exp):
        g = [t.cpu().numpy() for t in nn]
        return ((g[0].astype(np.uint32).astype(np.uint64) == exp[0]).all() and (g[2].astype(np.uint32).astype(np.uint64) == exp[2]).all()
                and (bits(g[1]) == bits(exp[1])).all() and (bits(g[3]) == bits(exp[3])).all())

    p1, fe1, nn1 = reference(c1, 0.2)
    p2, fe2, nn2 = reference(c2, 7.0)
    f1, f2 = torch.from_numpy(fe1).cuda(), torch.from_numpy(fe2).cuda()
    # the legitimate pair
    assert (u64(dens.calculate_populations_partial(t1, [0.2], variant=V)) == p1).all()
    assert same(dens.nearest_neighbors_partial(t1, f1, variant=V, stats_valid=True), nn1)
    assert (u64(dens.calculate_populations_partial(t1, [0.2], variant=V, stats_valid=True)) == p1).all()
    # a false claim: the workspace holds the statistics of c1, the calls are about c2
    assert same(dens.nearest_neighbors_partial(t2, f2, variant=V, stats_valid=True), nn2)
    assert (u64(dens.calculate_populations_partial(t2, [7.0], variant=V, stats_valid=True)) == p2).all()
    # the same buffer rewritten in place after fresh statistics of c2
    dens.calculate_populations_partial(t2, [7.0], variant=V)
    t2.copy_(t1)
    assert same(dens.nearest_neighbors_partial(t2, f1, variant=V, stats_valid=True), nn1)
    assert (u64(dens.calculate_populations_partial(t2, [0.2], variant=V, stats_valid=True)) == p1).all()


# ---- refusals ----------------------------------------------------------------------------------------------------

def test_refusals_are_error_codes(dens, oracle):
    """n_cols outside 9 .. 10 and segment calls are refused with an error code (RuntimeError), not an exit; the next
    valid call is still right"""
    import torch
    for d in (1, 8, 11, 64):
        ct = torch.from_numpy(gaussian_blobs(300, d, seed=d)).cuda()
        with pytest.raises(RuntimeError):
            dens.calculate_populations_partial(ct, [0.3], variant=V)
        fe = torch.zeros(300, dtype=torch.float32, device="cuda")
        with pytest.raises(RuntimeError):
            dens.nearest_neighbors_partial(ct, fe, variant=V)
    ct = torch.from_numpy(gaussian_blobs(300, 10, seed=10)).cuda()
    with pytest.raises(RuntimeError):
        dens.calculate_populations_segment(ct, [0.3], 0, 2, variant=V)
    with pytest.raises(RuntimeError):
        dens.nearest_neighbors_segment(ct, torch.zeros(300, dtype=torch.float32, device="cuda"), 1, 2, variant=V)
    check_full(dens, oracle, gaussian_blobs(700, 10, seed=11), [0.2, 0.15], what="after the refusals")


# ---- bounded seeded fuzz against the direct kernels --------------------------------------------------------------

def fuzz_case(dens, rng, case):
    import torch
    n = int(rng.choice([1, 2, 31, 32, 33, 64, 100, 257, 1000, 3000, 9000],
                       p=[.03, .03, .06, .06, .06, .06, .1, .2, .2, .12, .08]))
    d = int(rng.choice(DIMS))
    kind = int(rng.integers(0, 8))
    sig = float(rng.choice([0.02, 0.08, 0.3]))
    c = gaussian_blobs(n, d, seed=int(rng.integers(1, 1 << 30)), sigma=sig)
    if kind == 1:   # duplicates
        c[rng.integers(0, n, n // 3)] = c[rng.integers(0, n, n // 3)]
    if kind == 2:   # offsets (cancellation in the Gram form)
        c += np.float32(rng.choice([10.0, 1000.0, 1e4]))
    if kind == 3:   # tiny scale
        c *= np.float32(1e-3)
    if kind == 4:   # far from 1, the clamps of scale32_pop included
        c *= np.float32(rng.choice([1e-17, 1e-16, 1e-12, 1e-6, 1e4, 1e8]))
    sig_loc = None
    if kind >= 5 and n > 1:   # clusters over the plane of columns 0 / 1 (the spatial order of the population sweep)
        k = int(rng.choice([2, 3, 5, 12, 40, 90]))
        sig_loc = float(rng.choice([0.02, 0.08, 0.3]))
        spread = float(rng.choice([1.0, 4.0, 30.0, 300.0, 3000.0])) * sig_loc * np.sqrt(d)
        cen = np.zeros((k, d), dtype=np.float32)
        cen[:, :2] = rng.uniform(-spread, spread, size=(k, 2))
        if kind == 7:
            cen[:, 2:] = rng.uniform(-spread, spread, size=(k, d - 2)) * 0.1
        c = (cen[rng.integers(0, k, n)] + rng.normal(0.0, sig_loc, size=(n, d))).astype(np.float32)
        if kind == 6:             # a few far outliers
            c[rng.integers(0, n, max(1, n // 500))] += np.float32(50.0 * spread)
    c = np.ascontiguousarray(c, dtype=np.float32)
    ct = torch.from_numpy(c).cuda()
    scale = float(np.sqrt(d)) * (sig_loc if sig_loc is not None else float(c.std(axis=0).mean() if n > 1 else 1.0))
    radii = [float(x) for x in (scale * rng.uniform(0.05, 1.5, size=int(rng.integers(1, 18))))]
    lo = int(rng.integers(0, n))
    hi = int(rng.integers(lo, n + 1))
    if rng.random() < 0.4:
        lo, hi = 0, n
    what = f"case {case}: n={n} d={d} kind={kind} radii={radii} rows=[{lo},{hi})"
    ref_p = dens.calculate_populations_partial(ct, radii, lo, hi, variant="direct")
    fe = dens.calculate_free_energies(
        dens.calculate_populations_partial(ct, radii[:1], variant="direct")[0].contiguous())
    ref_n = dens.nearest_neighbors_partial(ct, fe, lo, hi, variant="direct")
    p = dens.calculate_populations_partial(ct, radii, lo, hi, variant=V)
    q = dens.nearest_neighbors_partial(ct, fe, lo, hi, variant=V)
    assert bool((p == ref_p).all()), f"populations, {what}"
    for x, y in zip(q, ref_n):
        assert bool((x.view(torch.int32) == y.view(torch.int32)).all()), f"neighbours, {what}"


@pytest.mark.parametrize("seed", [31, 32, 33])
def test_fuzz_against_direct(dens, seed):
    rng = np.random.default_rng(seed)
    for case in range(40):
        fuzz_case(dens, rng, case)


# ---- the other summation orders ----------------------------------------------------------------------------------

CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from clustering_amd import capi, density as dens
from clustering_amd.synth import gaussian_blobs
from oracle.oracle import Oracle
ORDER = sys.argv[2]
assert capi.lib.dc_hip_canon_order().decode() == ORDER
o = Oracle(order=ORDER)
bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
for d in (9, 10):
    rng = np.random.default_rng(d)
    r = float(np.sqrt(d) * 0.08 * 1.1)
    base = gaussian_blobs(1400, d, seed=90 + d)
    dup = np.concatenate([base, base[:600], base[100:200]])
    cases = [("scale 1e-17", gaussian_blobs(1300, d, seed=50 + d) * np.float32(1e-17), [r * 1e-17, 0.6 * r * 1e-17]),
             ("lattice", rng.integers(0, 4, (1200, d)) * 0.25, [0.25, 0.5, 0.3535534]),
             ("duplicates", dup[rng.permutation(dup.shape[0])], [0.2, 0.25]),
             ("offset +1e4", gaussian_blobs(1500, d, seed=110 + d, sigma=0.02) + np.float32(1e4), [0.02 * np.sqrt(d)])]
    for name, c, radii in cases:
        c = np.ascontiguousarray(c, dtype=np.float32)
        ct = torch.from_numpy(c).cuda()
        want = o.populations(c, radii)
        fe_want = o.free_energies(want[0])
        exp = o.nearest_neighbors(c, fe_want)
        p = dens.calculate_populations_partial(ct, radii, variant="mfma32")
        assert (p.cpu().numpy().astype(np.uint32).astype(np.uint64) == want).all(), (d, name, "pops")
        fe = dens.calculate_free_energies(p[0].contiguous())
        assert (bits(fe.cpu().numpy()) == bits(fe_want)).all(), (d, name, "fe")
        g = [t.cpu().numpy() for t in dens.nearest_neighbors_partial(ct, fe, variant="mfma32")]
        assert (g[0].astype(np.uint32).astype(np.uint64) == exp[0]).all() and (g[2].astype(np.uint32).astype(np.uint64) == exp[2]).all(), (d, name, "nn idx")
        assert (bits(g[1]) == bits(exp[1])).all() and (bits(g[3]) == bits(exp[3])).all(), (d, name, "nn d2")
print("ok")
"""


@pytest.mark.parametrize("order", ["avx", "fma"])
def test_other_order_library_at_the_edges(order):
    """the canonical re-check of band pairs (pop32_fix, exact_d2) in the summation order of the avx / fma libraries,
    on cases that force many band pairs, against the oracle of that order"""
    if not os.path.exists(os.path.join(ROOT, "clustering_amd", "lib_" + order, "libdcdensity.so")):
        pytest.fail(f"clustering_amd/lib_{order}/libdcdensity.so is missing: __graft_entry__.build() makes it")
    env = dict(os.environ, DC_CANON_ORDER=order)
    env.pop("DC_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, order], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
