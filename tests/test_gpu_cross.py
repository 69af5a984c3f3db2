"""GPU (-m gpu): the cross sweeps -- new frames measured against a reference trajectory (dc_hip_*_cross_dev,
clustering_amd.density.calculate_populations_against / nearest_reference / assign_frames) -- against exact values from
the CPU referees: the [n_q, n_r] block of the probe's pairwise d2 matrix (the reference's own loop shape) for
populations and neighbours, the oracle's populations of the union for large runs, the oracle's self sweeps for the
properties a cross sweep must share with them, and Python's math.log (the host libm) for the free energies."""
import numpy as np
import pytest

import fe_families
from crossref import (FLT_MAX, F32, bits, block_d2, expect_nn, expect_pops, fe_of, gpu, host, radius,
                      same_nn, sets, variants)
from clustering_amd.synth import gaussian_blobs

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 3, 4, 5, 9, 10, 16, 30, 33, 64, 65, 100, 401]


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


@pytest.fixture(scope="module")
def oracle():
    from clustering_amd import capi
    from oracle.oracle import Oracle
    return Oracle(order=capi.CANON_ORDER)


# ---- parity ---------------------------------------------------------------------------------------------------------
SHAPES = [(1037, 2311), (1, 33), (33, 1), (31, 32), (32, 31), (33, 33)]


@pytest.mark.parametrize("D", WIDTHS)
def test_parity_every_width(dens, probe, D):
    shapes = SHAPES if D <= 100 else [(300, 700), (1, 33), (33, 1)]
    for n_q, n_r in shapes:
        Q, R = sets(D, n_q, n_r, seed=D * 7 + n_q)
        d2 = block_d2(probe, Q, R)
        r0 = radius(D)
        radii = [r0, 0.5 * r0, 2.0 * r0]   # (unsorted)
        i_from, i_to = (n_q // 5, n_q - n_q // 7) if n_q > 8 else (0, n_q)
        pops_exp = expect_pops(d2, radii, i_from, i_to)
        rng = np.random.default_rng(D + n_r)
        fe_q = rng.normal(size=n_q).astype(np.float32)
        fe_r = rng.normal(size=n_r).astype(np.float32)
        nn_exp = expect_nn(d2, fe_q, fe_r, i_from, i_to)
        q, r = gpu(Q), gpu(R)
        for v in variants(D):
            pops = dens.calculate_populations_against(q, r, radii, i_from, i_to, variant=v)
            assert (host(pops) == pops_exp).all(), (D, n_q, n_r, v)
            got = dens.nearest_reference(q, r, gpu(fe_q), gpu(fe_r), i_from, i_to, variant=v)
            same_nn(got, nn_exp, (D, n_q, n_r, v))
            nn_only = dens.nearest_reference(q, r, i_from=i_from, i_to=i_to, variant=v)
            assert nn_only[2] is None and nn_only[3] is None
            same_nn(nn_only, nn_exp[:2], (D, n_q, n_r, v, "nn only"))


def test_query_equals_reference_gives_the_self_populations(dens, oracle):
    c = gaussian_blobs(20000, 10, seed=3)
    radii = [0.2, 0.1, 0.3]
    want = oracle.populations(c, radii)
    t = gpu(c)
    for v in variants(10):
        got = dens.calculate_populations_against(t, t, radii, variant=v)   # (the same buffer on both sides)
        assert (host(got).astype(np.uint64) == want).all(), v


@pytest.mark.parametrize("D", [10, 33, 401])
def test_same_buffer_on_both_sides_keeps_the_self_pair(dens, probe, D):
    """Against a reference that is the query buffer itself, every pair counts, the self pair included: radius 0 gives
    0 (a self sweep gives 1), and each frame's nearest reference is its lowest-index exact copy at d2 = 0 (a self sweep
    gives another frame).  Nothing may decide the mode by comparing the two pointers."""
    n = 777 if D <= 64 else 300
    c = gaussian_blobs(n, D, seed=D + 17)
    rng = np.random.default_rng(D)
    c[rng.integers(0, n, n // 8)] = c[rng.integers(0, n, n // 8)]   # exact copies, before and after their originals
    d2 = block_d2(probe, c, c)
    radii = [0.0, radius(D), 0.5 * radius(D)]
    pops_exp = expect_pops(d2, radii)
    assert (pops_exp[0] == 0).all()
    fe = rng.normal(size=n).astype(np.float32)
    nn_exp = expect_nn(d2, fe, fe)
    assert (nn_exp[1] == 0).all() and (nn_exp[0] <= np.arange(n)).all()
    t, f = gpu(c), gpu(fe)
    for v in variants(D):
        pops = dens.calculate_populations_against(t, t, radii, variant=v)
        assert (host(pops) == pops_exp).all(), (D, v)
        same_nn(dens.nearest_reference(t, t, f, f, variant=v), nn_exp, (D, v))
        same_nn(dens.nearest_reference(t, t, variant=v), nn_exp[:2], (D, v, "nn only"))


@pytest.mark.parametrize("family", sorted(fe_families.FAMILIES))
def test_copies_of_reference_frames(dens, oracle, family):
    """Q = R[S]: the populations are the self populations of S, the free energies against R's maximum are fe_R[S] bit
    for bit, and nn_hd is the oracle's self nn_hd of S"""
    D, r0 = 10, 0.2
    R = gaussian_blobs(3000, D, seed=11)
    rng = np.random.default_rng(5)
    R[rng.integers(0, 3000, 150)] = R[rng.integers(0, 3000, 150)]
    S = rng.permutation(3000)[:1111]
    Q = R[S]
    pops_r = oracle.populations(R, [r0])[0]
    fe_r = fe_families.make(family, R, pops_r, seed=1)
    exp = oracle.nearest_neighbors(R, fe_r)
    q, r = gpu(Q), gpu(R)
    for v in variants(D):
        pops_q = dens.calculate_populations_against(q, r, [r0], variant=v)[0].contiguous()
        assert (host(pops_q).astype(np.uint64) == pops_r[S]).all(), v
        fe_q = dens.calculate_free_energies_against(pops_q, int(pops_r.max()))
        assert (bits(host(fe_q)) == bits(oracle.free_energies(pops_r)[S])).all(), v
        got = dens.nearest_reference(q, r, gpu(fe_r[S]), gpu(fe_r), variant=v)
        assert (host(got[2]).astype(np.uint64) == exp[2][S]).all(), (family, v)
        assert (bits(host(got[3])) == bits(exp[3][S])).all(), (family, v)
        assert (host(got[1]) == 0).all(), v   # (every query has its own copy in R)


def test_free_energies_against_another_maximum(dens):
    import torch
    pops = np.array([0, 1, 2, 3, 7, 100, 101, 250, 999, 1000, 1001, 5000, 123456], dtype=np.int32)
    for mx in (1, 100, 1000, 77777):
        got = host(dens.calculate_free_energies_against(torch.from_numpy(pops).cuda(), mx))
        assert (bits(got) == bits(fe_of(pops, mx))).all(), mx
    assert np.isinf(got[0]) and got[0] > 0 and (got[pops > 77777] < 0).all()
    with pytest.raises(RuntimeError):
        dens.calculate_free_energies_against(torch.from_numpy(pops).cuda(), 0)


# ---- scale edges -----------------------------------------------------------------------------------------------------
def _check_pair(dens, probe, Q, R, radii, what):
    d2 = block_d2(probe, Q, R)
    rng = np.random.default_rng(len(Q))
    fe_q = rng.normal(size=len(Q)).astype(np.float32)
    fe_r = rng.normal(size=len(R)).astype(np.float32)
    pops_exp, nn_exp = expect_pops(d2, radii), expect_nn(d2, fe_q, fe_r)
    q, r = gpu(Q), gpu(R)
    for v in variants(Q.shape[1]):
        assert (host(dens.calculate_populations_against(q, r, radii, variant=v)) == pops_exp).all(), (what, v)
        same_nn(dens.nearest_reference(q, r, gpu(fe_q), gpu(fe_r), variant=v), nn_exp, (what, v))
    return pops_exp, nn_exp


@pytest.mark.parametrize("D", [3, 10, 30])
def test_scale_edges(dens, probe, D):
    rng = np.random.default_rng(D)
    R = (rng.normal(size=(1500, D)) * 0.02).astype(np.float32)
    # queries offset by +1e4 from a reference with sigma 0.02 (and some right on it)
    Q = (R[:700] + F32(1e4)).astype(np.float32)
    Q[::7] = R[:700:7] + (rng.normal(size=(100, D)) * 0.01).astype(np.float32)
    _check_pair(dens, probe, Q, R, [0.05, 0.02, 0.1], "offset 1e4")
    # queries a thousand units away: no populations, FE +inf, hd == nn
    Q = (rng.normal(size=(500, D)) * 0.02 + 1000.0).astype(np.float32)
    pops_exp, nn_exp = _check_pair(dens, probe, Q, R, [0.5], "far away")
    assert (pops_exp == 0).all()
    q, r = gpu(Q), gpu(R)
    for v in variants(D):
        pops = dens.calculate_populations_against(q, r, [0.5], variant=v)[0].contiguous()
        fe = host(dens.calculate_free_energies_against(pops, 17))
        assert np.isposinf(fe).all()
        nn = dens.nearest_reference(q, r, gpu(fe), gpu(np.zeros(len(R), np.float32)), variant=v)
        assert (host(nn[0]) == host(nn[2])).all() and (bits(host(nn[1])) == bits(host(nn[3]))).all(), v
    # a reference of tiny extent and queries of large extent, and the other way round
    tiny = (rng.normal(size=(900, D)) * 1e-3).astype(np.float32)
    large = (rng.normal(size=(800, D)) * 50.0).astype(np.float32)
    large[::5] = tiny[:160] * F32(3.0)
    _check_pair(dens, probe, large, tiny, [0.003, 1e-3, 30.0], "tiny reference")
    _check_pair(dens, probe, tiny, large, [0.003, 1e-3, 30.0], "tiny queries")
    # duplicated reference rows: the lowest index wins
    R2 = np.repeat(gaussian_blobs(400, D, seed=D), 3, axis=0)[np.random.default_rng(1).permutation(1200)]
    _, nn_exp = _check_pair(dens, probe, R2[::5].copy(), R2, [radius(D)], "duplicates")
    assert (nn_exp[1] == 0).all()


@pytest.mark.parametrize("D", [4, 10, 65])
def test_non_finite_rows_and_an_empty_reference(dens, probe, D):
    Q, R = sets(D, 700, 900, seed=D)
    Q[3, 0] = np.inf
    Q[10, D - 1] = np.nan
    R[5, 0] = -np.inf
    R[17, D // 2] = np.nan
    pops_exp, nn_exp = _check_pair(dens, probe, Q, R, [radius(D), 2 * radius(D)], "non-finite")
    assert (pops_exp[:, [3, 10]] == 0).all()
    assert not np.isin(nn_exp[0], [5, 17]).any() and not np.isin(nn_exp[2], [5, 17]).any()
    q = gpu(Q)
    empty = gpu(np.zeros((0, D), np.float32))
    for v in variants(D):
        assert (host(dens.calculate_populations_against(q, empty, [1.0, 2.0], variant=v)) == 0).all(), v
        fe0 = gpu(np.zeros(len(Q), np.float32))
        nn = dens.nearest_reference(q, empty, fe0, gpu(np.zeros(0, np.float32)), variant=v)
        for k in (0, 2):
            assert (host(nn[k]) == 1).all() and (host(nn[k + 1]) == FLT_MAX).all(), v


def test_refusals_leave_the_next_call_right(dens, probe):
    Q, R = sets(10, 300, 500, seed=2)
    d2 = block_d2(probe, Q, R)
    q, r = gpu(Q), gpu(R)
    for bad in ("pruned", "mfma32"):
        with pytest.raises(RuntimeError):
            dens.calculate_populations_against(q, r, [0.2], variant=bad)
        with pytest.raises(RuntimeError):
            dens.nearest_reference(q, r, variant=bad)
    import ctypes as C
    from clustering_amd import capi
    rad = (C.c_float * 1)(0.2)
    out = gpu(np.zeros(300, np.float32))   # (never written: the call is refused first)
    rc = capi.lib.dc_hip_populations_cross_dev(C.c_void_p(q.data_ptr()), 300, C.c_void_p(r.data_ptr()), 500, 10, rad,
                                               1, 0, 300, C.c_void_p(out.data_ptr()), None, 0,
                                               capi.VARIANT_AUTO | capi.FLAG_STATS_VALID, None)
    assert rc == -1
    Q65, R65 = sets(65, 50, 60, seed=3)
    with pytest.raises(RuntimeError):
        dens.calculate_populations_against(gpu(Q65), gpu(R65), [1.0], variant="mfma")
    with pytest.raises(RuntimeError):
        dens.nearest_reference(gpu(Q65), gpu(R65), variant="mfma")
    assert (host(dens.calculate_populations_against(q, r, [0.2], variant="mfma")) == expect_pops(d2, [0.2])).all()
    same_nn(dens.nearest_reference(q, r, variant="mfma"), expect_nn(d2)[:2], "after refusals")


def test_host_pointer_entry_points(probe):
    import ctypes as C
    from clustering_amd import capi
    Q, R = sets(9, 333, 777, seed=9)
    d2 = block_d2(probe, Q, R)
    rng = np.random.default_rng(0)
    fe_q, fe_r = rng.normal(size=333).astype(np.float32), rng.normal(size=777).astype(np.float32)
    radii = np.array([0.3, 0.1], np.float32)
    pops = np.zeros((2, 333), np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    capi.check(capi.lib.dc_hip_populations_cross(p(Q), 333, p(R), 777, 9, p(radii), 2, 10, 300, 0, p(pops)))
    assert (pops == expect_pops(d2, radii, 10, 300)).all()
    out = [np.zeros(333, np.uint32), np.zeros(333, np.float32), np.zeros(333, np.uint32), np.zeros(333, np.float32)]
    capi.check(capi.lib.dc_hip_nearest_neighbors_cross(p(Q), 333, p(R), 777, 9, p(fe_q), p(fe_r), 0, 333, 0,
                                                       *[p(a) for a in out]))
    exp = expect_nn(d2, fe_q, fe_r)
    for k in (0, 2):
        assert (out[k].astype(np.int64) == exp[k]).all() and (bits(out[k + 1]) == bits(exp[k + 1])).all()


# ---- end to end -------------------------------------------------------------------------------------------------------
def test_assign_frames_end_to_end(dens, oracle, probe):
    from oracle.oracle import ScreeningOracle
    so = ScreeningOracle()
    D, r0 = 6, 0.25
    c = gaussian_blobs(5000, D, seed=21)
    R, Q = c[:3500].copy(), c[3500:].copy()
    Q[::9] = R[:Q[::9].shape[0]]
    pops_r = oracle.populations(R, [r0])[0]
    fe_r = oracle.free_energies(pops_r)
    nn = oracle.nearest_neighbors(R, fe_r)
    fe_max = float(np.sort(fe_r)[len(fe_r) // 3])
    clust = so.screening(fe_r, nn[1], fe_max, R)
    states_r = so.sorted_names(so.assign_low_density(clust, nn[2], fe_r)).astype(np.int64)
    d2 = block_d2(probe, Q, R)
    pops_q = expect_pops(d2, [r0])[0]
    fe_q = fe_of(pops_q, int(pops_r.max()))
    exp = expect_nn(d2, fe_q, fe_r)
    none = len(R) + 1
    pick = np.where(exp[2] != none, exp[2], exp[0])
    want = np.where(pick != none, states_r[np.minimum(pick, len(R) - 1)], 0)
    for v in variants(D):
        got = dens.assign_frames(gpu(Q), gpu(R), r0, states_r, variant=v)
        assert (host(got["pops"]) == pops_q).all(), v
        assert got["max_pop"] == int(pops_r.max())
        assert (bits(host(got["fe"])) == bits(fe_q)).all(), v
        assert (bits(host(got["fe_ref"])) == bits(fe_r)).all(), v
        same_nn([got["nn_idx"], got["nn_d2"], got["hd_idx"], got["hd_d2"]], exp, v)
        assert (host(got["states"]) == want).all(), v
    assert (want != 0).any()


def test_large_run(dens, oracle):
    """200 000 queries against 1 000 000 reference frames at D = 10: three row ranges of 2000 queries against the
    oracle (populations of the union minus those of the queries alone; nearest reference frame as the oracle's
    nn_hd of the union with the queries at +inf free energy, so that only reference frames are candidates)"""
    import torch
    D, r0 = 10, 0.2
    c = gaussian_blobs(1_200_000, D, seed=77)
    Q, R = c[:200_000], c[200_000:]
    want = {}
    for lo in (0, 98_765, 198_000):
        hi = lo + 2000
        U = np.vstack([Q[lo:hi], R])
        pops = oracle.populations(U, [r0], 0, 2000)[0][:2000] - oracle.populations(Q[lo:hi], [r0])[0]
        fe = np.zeros(len(U), np.float32)
        fe[:2000] = np.inf
        exp = oracle.nearest_neighbors(U, fe, 0, 2000)
        want[lo] = (pops, exp[2][:2000].astype(np.int64) - 2000, exp[3][:2000])
    q, r = gpu(Q), gpu(R)
    for v in variants(D):
        pops = host(dens.calculate_populations_against(q, r, [r0], variant=v)[0])
        nn = dens.nearest_reference(q, r, variant=v)
        nn_i, nn_d = host(nn[0]), host(nn[1])
        for lo, (p_exp, i_exp, d_exp) in want.items():
            hi = lo + 2000
            assert (pops[lo:hi].astype(np.uint64) == p_exp).all(), (v, lo)
            assert (nn_i[lo:hi].astype(np.int64) == i_exp).all(), (v, lo)
            assert (bits(nn_d[lo:hi]) == bits(d_exp)).all(), (v, lo)
        del nn
        torch.cuda.empty_cache()
