"""GPU: the matrix-core sweeps for rows of 257..1024 columns (density.calculate_populations_xwide, nearest_neighbors_xwide,
their cross forms and assign_frames_xwide), bit for bit: populations, nn_idx, nn_d2 bits, hd_idx, hd_d2 bits.  The self sweeps
are held to the CPU oracle (the 1 500-row cases, beyond the size the oracle is asked for here, and the cross sweeps to the
direct kernels, which are the oracle's image at every width).  Every finite case first asserts that the matrix-core kernel
answered -- tiles > 0 and MFMAs > 0 from the info call -- so that a silent fall-back cannot pass.
Cases and their premises: tests/xwideref.py, tests/test_xwide_cases.py."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import xwideref as xw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def dens():
    import torch
    assert torch.cuda.is_available()
    from clustering_amd import density
    return density


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def u64(t):
    return t.cpu().numpy().astype(np.uint32).astype(np.uint64)


def gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def radii_for(n_cols, k=3):
    """k radii around the intra-blob distance of synth.gaussian_blobs (d2 ~ 2 sigma^2 D), not sorted"""
    base = float(np.sqrt(2 * 0.08 * 0.08 * n_cols))
    return [base * f for f in (1.0, 0.9, 1.08, 0.95, 1.2, 0.8, 1.02, 0.85)[:k]]


@functools.lru_cache(maxsize=None)
def blob_reference(n_rows, n_cols, k):
    """(coords, radii, populations, free energies of the first radius, neighbours): computed once per shape"""
    from oracle.oracle import Oracle
    o = Oracle()
    c = xw.blobs(n_rows, n_cols)
    radii = radii_for(n_cols, k)
    pops = o.populations(c, radii)
    fe = o.free_energies(pops[0])
    return c, radii, pops, fe, o.nearest_neighbors(c, fe)


def answered(info, n_cols, what):
    tiles, mfmas, _ = info
    assert tiles > 0 and mfmas > 0, (what, "the matrix-core kernel did not answer")
    assert mfmas == xw.nm_for(n_cols) * tiles, (what, tiles, mfmas)


def check_pops(dens, oracle, c, radii, lo=0, hi=None, want=None, finite=True):
    hi = len(c) if hi is None else hi
    ct = gpu(c)
    got = dens.calculate_populations_xwide(ct, radii, lo, hi)
    info = dens.xwide_sweep_info(ct.device)
    if finite and hi > lo:
        answered(info, c.shape[1], ("populations", c.shape))
    if want is None:
        want = oracle.populations(c, radii, lo, hi)
    assert (u64(got) == want).all(), ("populations", c.shape, radii, lo, hi)
    return info


def same_nn(got, want, what):
    assert (u64(got[0]) == want[0]).all(), ("nn_idx", what)
    assert (bits(got[1].cpu().numpy()) == bits(want[1])).all(), ("nn_d2", what)
    assert (u64(got[2]) == want[2]).all(), ("hd_idx", what)
    assert (bits(got[3].cpu().numpy()) == bits(want[3])).all(), ("hd_d2", what)


def check_nn(dens, oracle, c, fe, lo=0, hi=None, want=None, finite=True):
    hi = len(c) if hi is None else hi
    ct = gpu(c)
    got = dens.nearest_neighbors_xwide(ct, gpu(np.asarray(fe, dtype=np.float32)), lo, hi)
    info = dens.xwide_sweep_info(ct.device)
    if finite and hi > lo:
        answered(info, c.shape[1], ("neighbours", c.shape))
    if want is None:
        want = oracle.nearest_neighbors(c, fe, lo, hi)
    same_nn(got, want, (c.shape, lo, hi))
    return info


# ---- 1, 2, 3: widths, row counts, row ranges -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols", xw.COLS)
def test_every_width_on_both_sides_of_every_seam(dens, oracle, n_cols):
    c, radii, pops, fe, nn = blob_reference(200, n_cols, 3)
    info = check_pops(dens, oracle, c, radii, want=pops)
    assert info[0] == xw.tile_pairs(2, 2)
    check_nn(dens, oracle, c, fe, want=nn)


@pytest.mark.parametrize("n_rows", xw.ROWS)
def test_row_counts_from_one_frame_to_two_reference_shares(dens, oracle, n_rows):
    c, radii, pops, fe, nn = blob_reference(n_rows, 300, 1)
    info_p = check_pops(dens, oracle, c, radii, want=pops)
    info_n = check_nn(dens, oracle, c, fe, want=nn)
    b = xw.blocks(n_rows)
    assert info_p[:2] == (xw.tile_pairs(b, b), 57 * xw.tile_pairs(b, b)) and info_n[:2] == info_p[:2], "57 MFMAs per tile pair at 300 columns"
    if n_rows == 1:
        assert int(pops[0][0]) == 1 and int(nn[0][0]) == 2 and nn[1][0] == FLT_MAX
    if n_rows == 2100:
        assert xw.shares(b) == 2 and info_p[0] == 17 * 17 * 16, "17 reference blocks in two shares: every block still met once"


@pytest.mark.parametrize("lo,hi", [(37, 171), (128, 256), (0, 1), (299, 300), (33, 290), (5, 5), (300, 300)])
def test_row_ranges_that_start_and_end_inside_tiles(dens, oracle, lo, hi):
    c, radii, _, fe, _ = blob_reference(300, 300, 3)
    info_p = check_pops(dens, oracle, c, radii, lo, hi)
    info_n = check_nn(dens, oracle, c, fe, lo, hi)
    if lo == hi:
        assert info_p == (0, 0, 0) and info_n == (0, 0, 0), "nothing swept: zeros / none, and counters that say so"
    else:
        q_blocks = (hi + 127) // 128 - lo // 128
        assert info_p[0] == xw.tile_pairs(q_blocks, 3) and info_n[0] == info_p[0]


# ---- 4: radii at the edges ------------------------------------------------------------------------------------------------------
def test_radii_in_any_order_and_at_the_edges(dens, oracle):
    c, r_edge, groups = xw.boundary_case(300, 300)
    base = float(np.sqrt(2 * 0.3 * 0.3 * 300))
    one = [r_edge]
    three = [base * 1.1, r_edge, base * 0.9]
    eight = [base, 1e30, 0.0, r_edge, 1e-3, base * 0.8, float(np.nextafter(np.float32(r_edge), np.float32(4))), base * 1.3]
    eleven = eight + [base * 1.05, base * 0.7, r_edge]
    infos = {}
    for radii in (one, three, eight, eleven):
        want = oracle.populations(c, radii)
        infos[len(radii)] = info = check_pops(dens, oracle, c, radii, want=want)
        assert info[2] > 0, "pairs exactly on a radius can only be decided by the exact path"
        k = radii.index(r_edge)
        for a, b, cc, d in groups:
            assert int(want[k][a]) >= 2   # (the pair one ulp inside the radius counts, the one on it does not)
    want = oracle.populations(c, eight)
    assert (want[eight.index(1e30)] == len(c)).all() and (want[eight.index(0.0)] == 1).all()
    assert int(want[eight.index(1e-3)].max()) <= 4   # (only the rows the groups copied)
    above = eight.index(float(np.nextafter(np.float32(r_edge), np.float32(4))))
    for a, b, cc, d in groups:
        assert int(want[above][a]) >= int(want[eight.index(r_edge)][a]) + 1, "one ulp above the radius the pair on it counts"
    # 300 rows: 3 x 3 blocks of 16 tile pairs, 57 MFMAs each; eleven radii are two launches and the counters cover both
    assert infos[8][:2] == (144, 144 * 57) and infos[11][:2] == (2 * 144, 2 * 144 * 57)


# ---- 5: what reaches the exact path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols", xw.BAND_COLS)
def test_exact_path_share_of_the_blob_case(dens, n_cols):
    """populations: at most the pairs the band can defer, counted on the CPU (xwideref.band_case); neighbours: some, and
    at most 5 % of the evaluated pairs.  Results against the direct kernels (1 500 x 1024 is beyond the oracle call this
    file allows itself)."""
    import torch
    c, radii, bound, pairs = xw.band_case(n_cols)
    ct = gpu(c)
    got = dens.calculate_populations_xwide(ct, radii)
    tiles, mfmas, exact = info = dens.xwide_sweep_info(ct.device)
    answered(info, n_cols, "band case")
    want = dens.calculate_populations_partial(ct, radii, variant="direct")
    assert bool((got == want).all())
    print(f"D={n_cols} populations: {tiles} tile pairs, {mfmas} MFMAs, {exact} exact pairs; the band allows {bound} of {pairs} "
          f"({100.0 * exact / pairs:.4f} % against {100.0 * bound / pairs:.4f} %)")
    assert tiles == xw.tile_pairs(12, 12)
    assert exact <= bound, (exact, bound)
    fe = dens.calculate_free_energies(want[0].contiguous())
    nn = dens.nearest_neighbors_xwide(ct, fe)
    tiles, mfmas, exact = info = dens.xwide_sweep_info(ct.device)
    answered(info, n_cols, "band case neighbours")
    for x, y in zip(nn, dens.nearest_neighbors_partial(ct, fe, variant="direct")):
        assert bool((x.view(torch.int32) == y.view(torch.int32)).all())
    print(f"D={n_cols} neighbours: {exact} exact pairs = {100.0 * exact / (1024 * tiles):.4f} % of the evaluated pairs")
    assert 0 < exact <= 0.05 * 1024 * tiles


# ---- 6, 7, 8: scaled data, free energies, flagged data --------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["scale 1e-3", "scale 1e3", "offset 1e4"])
def test_scaled_and_offset_data(dens, oracle, what):
    c, radii, _, _, _ = blob_reference(300, 300, 3)
    if what == "offset 1e4":
        c2, r2 = (c + np.float32(10000.0)).astype(np.float32), radii
    else:
        f = np.float32(1e-3 if what == "scale 1e-3" else 1e3)
        c2, r2 = (c * f).astype(np.float32), [float(np.float32(r) * f) for r in radii]
    c2 = np.ascontiguousarray(c2)
    pops = oracle.populations(c2, r2)
    check_pops(dens, oracle, c2, r2, want=pops)
    check_nn(dens, oracle, c2, oracle.free_energies(pops[0]))


def fe_kinds(n):
    rng = np.random.default_rng(21)
    kinds = dict(xw.fe_families(n))
    some_inf = rng.normal(0.0, 1.0, n).astype(np.float32)
    some_inf[rng.integers(0, n, 9)] = np.inf
    some_inf[rng.integers(0, n, 9)] = -np.inf
    kinds["some +-inf"] = some_inf
    kinds["all +inf"] = np.full(n, np.inf, dtype=np.float32)
    return kinds


@pytest.mark.parametrize("kind", ["equal", "ties", "zeros", "some +-inf", "all +inf", "populations", "one NaN"])
def test_free_energies_of_any_kind(dens, oracle, kind):
    c, stars, dups = xw.ties_case(300, 300)
    if kind == "populations":
        fe = oracle.free_energies(oracle.populations(c, [radii_for(300, 1)[0]])[0])
    elif kind == "one NaN":
        fe = xw.fe_families(len(c))["ties"].copy()
        fe[77] = np.nan
    else:
        fe = fe_kinds(len(c))[kind]
    want = oracle.nearest_neighbors(c, fe)
    info = check_nn(dens, oracle, c, fe, want=want, finite=kind != "one NaN")
    for q, ring in stars:
        assert int(want[0][q]) == min(ring), "the lowest row of a tie"
    for copy, orig in dups:
        assert want[1][copy] == 0.0 and want[1][orig] == 0.0
    if kind in ("equal", "all +inf"):
        assert (want[2] == len(c) + 1).all() and (want[3] == FLT_MAX).all(), "no frame of lower free energy anywhere"
    if kind == "one NaN":
        assert info == (0, 0, 0), "a NaN free energy flags the data: the direct kernel answers"


@pytest.mark.parametrize("n_cols", [300, 500])
@pytest.mark.parametrize("flaw", ["nan cell", "inf cell", "overflow row"])
def test_flagged_data_is_answered_by_the_direct_kernels(dens, oracle, flaw, n_cols):
    """300 columns: the generic direct kernel behind the gate; 500: the column-chunked one"""
    c, radii, pops, fe, nn = blob_reference(300, n_cols, 3)
    bad = c.copy()
    if flaw == "nan cell":
        bad[131, 7] = np.nan
    elif flaw == "inf cell":
        bad[40, n_cols - 1] = np.inf
    else:
        bad[200, :] = np.float32(1.0e18)   # |x|^2 = n_cols 1e36: beyond the 1e36 the Gram form is trusted to (at 500 columns: +inf)
    with np.errstate(invalid="ignore", over="ignore"):
        want_p = oracle.populations(bad, radii)
        want_n = oracle.nearest_neighbors(bad, fe, 10, 290)
    ct, ft = gpu(bad), gpu(fe)
    got = dens.calculate_populations_xwide(ct, radii)
    assert dens.xwide_sweep_info(ct.device) == (0, 0, 0)
    assert (u64(got) == want_p).all(), flaw
    got = dens.nearest_neighbors_xwide(ct, ft, 10, 290)
    assert dens.xwide_sweep_info(ct.device) == (0, 0, 0)
    same_nn(got, want_n, flaw)
    # ... and the next call on clean data in the same workspace runs on the matrix cores again
    check_pops(dens, oracle, c, radii, want=pops)
    check_nn(dens, oracle, c, fe, want=nn)


def test_the_gated_fallback_stands_down_on_clean_data(dens):
    """Beyond 400 columns the fallback behind the gate is the column-chunked direct kernel.  Were it to run on clean data
    as well, it would answer again with the same values -- no comparison of results can see that, only the time: the call
    would then cost the direct sweep and more.  Measured at 100 000 x 512, the direct sweep takes 5.6 x the matrix-core call
    (DESIGN.md 4.31); the condition here is a generous half, on the best of three calls each."""
    import time
    import torch
    c = gpu(xw.blobs(20000, 512))
    r = radii_for(512, 1)

    def best_ms(fn):
        fn()
        best = float("inf")
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) * 1e3)
        return best

    xwide = best_ms(lambda: dens.calculate_populations_xwide(c, r))
    answered(dens.xwide_sweep_info(c.device), 512, "gate")
    direct = best_ms(lambda: dens.calculate_populations_partial(c, r, variant="direct"))
    print(f"20 000 x 512: matrix cores {xwide:.2f} ms, direct {direct:.2f} ms")
    assert xwide < 0.5 * direct, (xwide, direct)


# ---- 9: one workspace -----------------------------------------------------------------------------------------------------------
def test_both_sweeps_in_one_workspace_in_either_order(dens, oracle):
    import torch
    from clustering_amd import capi
    c, radii, pops, fe, nn = blob_reference(300, 300, 3)
    n, d = c.shape
    ct, ft = gpu(c), gpu(fe)
    need = capi.lib.dc_hip_xwide_workspace_bytes(n, d, len(radii))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rad = np.ascontiguousarray(radii, dtype=np.float32)
    p = lambda t: C.c_void_p(t.data_ptr())

    def info():
        t, m, e = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        capi.check(capi.lib.dc_hip_wide_info_dev(p(ws), C.byref(t), C.byref(m), C.byref(e), None))
        return t.value, m.value, e.value

    def populations():
        out = torch.full((len(radii), n), -1, dtype=torch.int32, device="cuda")
        capi.check(capi.lib.dc_hip_populations_xwide_dev(p(ct), n, d, rad.ctypes.data_as(C.POINTER(C.c_float)), len(radii), 0, n,
                                                         p(out), p(ws), need, None))
        torch.cuda.synchronize()
        assert (u64(out) == pops).all()
        assert info()[:2] == (144, 57 * 144)

    def neighbours():
        o = [torch.full((n,), -1, dtype=torch.int32, device="cuda"), torch.full((n,), -1.0, device="cuda"),
             torch.full((n,), -1, dtype=torch.int32, device="cuda"), torch.full((n,), -1.0, device="cuda")]
        capi.check(capi.lib.dc_hip_nearest_neighbors_xwide_dev(p(ct), n, d, p(ft), 0, n, p(o[0]), p(o[1]), p(o[2]), p(o[3]),
                                                               p(ws), need, None))
        torch.cuda.synchronize()
        same_nn(o, nn, "one workspace")
        t, m, e = info()
        assert (t, m) == (144, 57 * 144) and e > 0

    for order in ((populations, neighbours), (neighbours, populations), (neighbours, neighbours, populations, populations)):
        for call in order:
            call()


# ---- 10, 11: the cross sweeps ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cross_sets(n_cols, n_q, n_r):
    """queries and reference from the same blobs; where the reference has the rows for it, reference rows lo < hi are
    duplicates and query q is a copy of them: d2 = 0 to both, a tie the lower row wins -> (Q, R, fe_q, fe_r, tie)"""
    R = xw.blobs(n_r, n_cols, seed=31 + n_r).copy()
    Q = xw.blobs(n_q, n_cols, seed=57 + n_q).copy()
    tie = None
    if n_r >= 200:
        lo, hi, q = 70, n_r - 3, n_q // 2
        R[hi] = R[lo]
        Q[q] = R[lo]
        tie = (q, lo, hi)
    rng = np.random.default_rng(n_q + 7 * n_r)
    fe_q = (rng.integers(0, 6, n_q) * 0.5).astype(np.float32)
    fe_r = (rng.integers(0, 6, n_r) * 0.5).astype(np.float32)
    return np.ascontiguousarray(Q), np.ascontiguousarray(R), fe_q, fe_r, tie


def check_cross(dens, n_cols, n_q, n_r, lo=0, hi=None):
    import torch
    Q, R, fe_q, fe_r, tie = cross_sets(n_cols, n_q, n_r)
    q, r, fq, fr = gpu(Q), gpu(R), gpu(fe_q), gpu(fe_r)
    radii = radii_for(n_cols, 3)
    hi_ = n_q if hi is None else hi
    q_blocks = (hi_ + 127) // 128 - lo // 128
    tiles = xw.tile_pairs(q_blocks, xw.blocks(n_r))
    what = (n_cols, n_q, n_r, lo, hi)
    got = dens.calculate_populations_against_xwide(q, r, radii, lo, hi)
    info = dens.xwide_against_info(q.device)
    answered(info, n_cols, what)
    assert info[0] == tiles, (what, info, tiles)
    assert bool((got == dens.calculate_populations_against(q, r, radii, lo, hi, variant="direct")).all()), what
    for with_fe in (True, False):
        nn = dens.nearest_reference_xwide(q, r, fq if with_fe else None, fr if with_fe else None, lo, hi)
        info = dens.xwide_against_info(q.device)
        answered(info, n_cols, what)
        assert info[0] == tiles, (what, info, tiles)
        want = dens.nearest_reference(q, r, fq if with_fe else None, fr if with_fe else None, lo, hi, variant="direct")
        if not with_fe:
            assert nn[2] is None and nn[3] is None, "without free energies there is no hd"
        for x, y in zip(nn[:4 if with_fe else 2], want):
            assert bool((x.view(torch.int32) == y.view(torch.int32)).all()), what
        if tie is not None and lo <= tie[0] < hi_:
            assert int(nn[0][tie[0]]) == tie[1] and float(nn[1][tie[0]]) == 0.0, "two duplicate reference rows tie: the lower row answers"


@pytest.mark.parametrize("n_cols", [257, 512, 1024])
@pytest.mark.parametrize("n_q,n_r", [(1, 1), (1, 300), (300, 1), (129, 257), (700, 1500)])
def test_cross_sweeps_against_the_direct_kernels(dens, n_cols, n_q, n_r):
    check_cross(dens, n_cols, n_q, n_r)


@pytest.mark.parametrize("lo,hi", [(37, 171), (128, 129), (699, 700), (5, 5)])
def test_cross_sweeps_over_a_query_range_inside_tiles(dens, lo, hi):
    import torch
    if lo < hi:
        check_cross(dens, 512, 700, 1500, lo, hi)
        return
    Q, R, fe_q, fe_r, _ = cross_sets(512, 700, 1500)
    q, r = gpu(Q), gpu(R)
    got = dens.calculate_populations_against_xwide(q, r, radii_for(512, 3), lo, hi)
    assert int(got.abs().sum()) == 0 and dens.xwide_against_info(q.device) == (0, 0, 0)
    nn = dens.nearest_reference_xwide(q, r, gpu(fe_q), gpu(fe_r), lo, hi)
    assert dens.xwide_against_info(q.device) == (0, 0, 0)
    assert bool((nn[0] == 1501).all()) and bool((nn[2] == 1501).all()) and bool((nn[1] == FLT_MAX).all()) and bool((nn[3] == FLT_MAX).all())


def test_assign_frames_xwide_equals_assign_frames(dens):
    import torch
    n_q, n_r, d = 700, 1500, 300
    R, Q = xw.blobs(n_r, d, seed=5), xw.blobs(n_q, d, seed=6)
    q, r = gpu(Q), gpu(R)
    radius = radii_for(d, 1)[0]
    states_r = (np.arange(n_r) % 5 + 1).astype(np.int32)
    got = dens.assign_frames_xwide(q, r, radius, states_r)
    assert dens.xwide_against_info(q.device)[0] == xw.tile_pairs(xw.blocks(n_q), xw.blocks(n_r))
    assert dens.xwide_sweep_info(q.device)[0] == xw.tile_pairs(xw.blocks(n_r), xw.blocks(n_r))
    ref = dens.assign_frames(q, r, radius, states_r)
    assert set(got) == set(ref)
    for key, val in ref.items():
        if key == "max_pop":
            assert got[key] == val
        else:
            assert got[key].dtype == val.dtype and got[key].shape == val.shape, key
            assert bool((got[key].view(torch.int32) == val.view(torch.int32)).all()), key
    assert int((got["states"] == 0).sum()) == 0 and got["max_pop"] > 1


@pytest.mark.parametrize("n_cols", [256, 1025])
def test_other_widths_raise(dens, n_cols):
    import torch
    from clustering_amd import capi
    c = torch.zeros((40, n_cols), dtype=torch.float32, device="cuda")
    fe = torch.zeros(40, device="cuda")
    with pytest.raises(capi.DensityLibraryError):
        dens.calculate_populations_xwide(c, [1.0])
    with pytest.raises(capi.DensityLibraryError):
        dens.nearest_neighbors_xwide(c, fe)
    for call in (lambda: dens.calculate_populations_against_xwide(c, c, [1.0]), lambda: dens.nearest_reference_xwide(c, c),
                 lambda: dens.assign_frames_xwide(c, c, 1.0, np.ones(40, dtype=np.int32))):
        with pytest.raises(ValueError):
            call()


# ---- 12: the libraries of the other summation orders ------------------------------------------------------------------------------
CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from clustering_amd import capi, density as dens
from oracle.oracle import Oracle
import xwideref as xw
ORDER = sys.argv[2]
assert capi.lib.dc_hip_canon_order().decode() == ORDER
o = Oracle(order=ORDER)
bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
u64 = lambda t: t.cpu().numpy().astype(np.uint32).astype(np.uint64)
n, d = 300, 300
for c, radii in ((xw.ties_case(n, d)[0], [float(np.sqrt(0.0128 * d)) * f for f in (1.0, 0.9, 1.1)]),
                 (xw.boundary_case(n, d)[0], [xw.wideref.BOUNDARY_RADIUS, float(np.sqrt(0.18 * d))])):
    ct = torch.from_numpy(c).cuda()
    want = o.populations(c, radii)
    got = dens.calculate_populations_xwide(ct, radii)
    t, m, e = dens.xwide_sweep_info(ct.device)
    assert t == 144 and m == 57 * t, (t, m)
    assert (u64(got) == want).all(), "pops"
    fe = o.free_energies(want[0])
    exp = o.nearest_neighbors(c, fe)
    g = dens.nearest_neighbors_xwide(ct, torch.from_numpy(fe).cuda())
    assert dens.xwide_sweep_info(ct.device)[0] == 144
    assert (u64(g[0]) == exp[0]).all() and (u64(g[2]) == exp[2]).all(), "nn idx"
    assert (bits(g[1].cpu().numpy()) == bits(exp[1])).all() and (bits(g[3].cpu().numpy()) == bits(exp[3])).all(), "nn d2"
    q = torch.from_numpy(np.ascontiguousarray(c[:130])).cuda()
    x = dens.calculate_populations_against_xwide(q, ct, radii)
    assert dens.xwide_against_info(q.device)[0] == 2 * 3 * 16
    assert bool((x == dens.calculate_populations_against(q, ct, radii, variant="direct")).all()), "cross pops"
print("ok")
"""


@pytest.mark.parametrize("order", ["avx", "fma"])
def test_the_libraries_of_the_other_summation_orders(order):
    if not os.path.exists(os.path.join(ROOT, "clustering_amd", "lib_" + order, "libdcdensity.so")):
        pytest.fail(f"clustering_amd/lib_{order}/libdcdensity.so is missing: __graft_entry__.build() makes it")
    env = dict(os.environ, DC_CANON_ORDER=order)
    env.pop("DC_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, order], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
