"""GPU: the cross form of the wide matrix-core sweeps (density.calculate_populations_against_wide, nearest_reference_wide,
assign_frames_wide; 65..256 columns) against the probe's canonical d2 (the [n_q, n_r] block of the union,
tests/crossref.py), bit for bit: populations, indices, d2 bits.  Every finite, non-empty case first asserts that the
matrix-core kernel answered -- wide_against_info: tile pairs > 0 and nm_for(D) MFMAs per tile pair -- a silent fall-back
to the direct kernels would otherwise pass.  Cases: tests/crosswideref.py (their conditions are checked on the CPU by
tests/test_cross_wide_cases.py)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import crossref
import crosswideref as cw
import wideref
from crossref import bits, block_d2, expect_nn, expect_pops, gpu, host, same_nn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def dens():
    import torch
    assert torch.cuda.is_available()
    from clustering_amd import density
    return density


@functools.lru_cache(maxsize=None)
def the_probe():
    from clustering_amd import capi
    from oracle.oracle import Probe
    return Probe(capi.CANON_ORDER)


@functools.lru_cache(maxsize=None)
def sets_case(n_cols, n_q, n_r):
    """(Q, R, d2) of crossref.sets -- duplicates between and within the sets included -- computed once per shape"""
    Q, R = crossref.sets(n_cols, n_q, n_r, seed=n_cols + n_q + 3 * n_r)
    return Q, R, block_d2(the_probe(), Q, R)


def same_pops(got, want, what):
    g = host(got)
    if not (g == want).all():
        bad = np.argwhere(g != want)
        k, i = bad[0]
        pytest.fail(f"pops {what}: {len(bad)} entries differ, e.g. radius {k} query {i}: {g[k, i]} != {want[k, i]}")


def answered(dens, dev, n_cols, what, expect_tiles=None):
    """the matrix-core kernel answered the last cross-wide call: tile pairs, and nm_for(D) MFMAs for each"""
    tiles, mfmas, exact = dens.wide_against_info(dev)
    assert tiles > 0 and mfmas == cw.nm_for(n_cols) * tiles, (what, "the matrix-core kernel did not answer", tiles, mfmas)
    if expect_tiles is not None:
        assert tiles == expect_tiles, (what, tiles, expect_tiles)
    return tiles, mfmas, exact


def check_pops(dens, Q, R, d2, radii, lo=0, hi=None, finite=True, launches=None, what=""):
    q, r = gpu(Q), gpu(R)
    got = dens.calculate_populations_against_wide(q, r, radii, lo, hi)
    info = dens.wide_against_info(q.device)
    hi_ = len(Q) if hi is None else hi
    if finite and hi_ > lo and len(R) and len(radii):
        launches = -(-len(radii) // 8) if launches is None else launches
        info = answered(dens, q.device, Q.shape[1], what, launches * cw.tile_pairs(len(Q), len(R), lo, hi))
    same_pops(got, expect_pops(d2, radii, lo, hi), (what, Q.shape, R.shape, radii, lo, hi))
    return info


def check_nn(dens, Q, R, d2, fe_q, fe_r, lo=0, hi=None, finite=True, what=""):
    q, r = gpu(Q), gpu(R)
    with_fe = fe_q is not None
    got = dens.nearest_reference_wide(q, r, gpu(fe_q) if with_fe else None, gpu(fe_r) if with_fe else None, lo, hi)
    info = dens.wide_against_info(q.device)
    hi_ = len(Q) if hi is None else hi
    if finite and hi_ > lo and len(R):
        info = answered(dens, q.device, Q.shape[1], what, cw.tile_pairs(len(Q), len(R), lo, hi))
    if not with_fe:
        assert got[2] is None and got[3] is None
    same_nn(got, expect_nn(d2, fe_q, fe_r, lo, hi), (what, Q.shape, R.shape, lo, hi))
    return info


def check_both(dens, Q, R, d2, radii, lo=0, hi=None, what=""):
    fe_q, fe_r = cw.fe_pair(len(Q), len(R))
    ip = check_pops(dens, Q, R, d2, radii, lo, hi, what=what)
    return ip, check_nn(dens, Q, R, d2, fe_q, fe_r, lo, hi, what=what)


@pytest.mark.parametrize("n_cols", wideref.COLS)
def test_column_counts_on_both_sides_of_every_seam(dens, n_cols):
    Q, R, d2 = sets_case(n_cols, 130, 200)
    check_both(dens, Q, R, d2, cw.radii_for(n_cols, 3))


@pytest.mark.parametrize("n_q,n_r", [(1, 1), (1, 300), (300, 1), (31, 129), (129, 31), (33, 127), (128, 128), (130, 1100),
                                     (40, 2100), (2100, 40)])
def test_rectangles_in_both_orientations_and_every_padding(dens, n_q, n_r):
    Q, R, d2 = sets_case(100, n_q, n_r)
    radii = cw.radii_for(100, 1)
    info_p, info_n = check_both(dens, Q, R, d2, radii)
    assert info_p[1] == 19 * info_p[0], "19 MFMAs per tile pair at 100 columns"
    if (n_q, n_r) == (1, 1):
        got = dens.nearest_reference_wide(gpu(Q), gpu(R))
        assert int(got[0][0]) == 0 and bits(host(got[1]))[0] == bits(d2[0, :1])[0], "the only reference is the neighbour, whatever it is"


@pytest.mark.parametrize("n_q,n_r", [(40, 0), (0, 40), (0, 0)])
def test_an_empty_side_gives_zeros_and_none(dens, n_q, n_r):
    import torch
    # (a call before it leaves counters behind that the empty call must not keep)
    Q0, R0, d20 = sets_case(100, 33, 127)
    check_pops(dens, Q0, R0, d20, cw.radii_for(100, 1))
    Q, R = np.zeros((n_q, 100), dtype=np.float32), np.zeros((n_r, 100), dtype=np.float32)
    q, r = torch.from_numpy(Q).cuda(), torch.from_numpy(R).cuda()
    got = dens.calculate_populations_against_wide(q, r, [0.5, 1e30])
    assert got.shape == (2, n_q) and int(got.abs().sum()) == 0
    assert dens.wide_against_info(q.device) == (0, 0, 0)
    check_nn(dens, Q0, R0, d20, None, None)
    fe_q, fe_r = torch.zeros(n_q, device="cuda"), torch.zeros(n_r, device="cuda")
    for with_fe in (False, True):
        nn = dens.nearest_reference_wide(q, r, fe_q if with_fe else None, fe_r if with_fe else None)
        assert dens.wide_against_info(q.device) == (0, 0, 0)
        for idx, dd in ((nn[0], nn[1]),) + (((nn[2], nn[3]),) if with_fe else ()):
            assert idx.shape == (n_q,) and bool((idx == n_r + 1).all()) and bool((dd == FLT_MAX).all())


@pytest.mark.parametrize("lo,hi", [(37, 171), (128, 256), (0, 1), (299, 300), (5, 5)])
def test_row_ranges_that_start_and_end_inside_tiles_and_blocks(dens, lo, hi):
    Q, R, d2 = sets_case(100, 300, 200)
    info_p, info_n = check_both(dens, Q, R, d2, cw.radii_for(100, 3), lo, hi)
    if lo == hi:
        assert info_p == (0, 0, 0) and info_n == (0, 0, 0), "nothing swept: zeros / none, and counters that say so"


def test_radii_in_any_order_at_the_edges_and_beyond_one_launch(dens):
    Q, R, r_edge, groups = cw.boundary_sets(300, 300, 80)
    d2 = block_d2(the_probe(), Q, R)
    base = float(np.sqrt(2 * 0.3 * 0.3 * 80))
    one = [r_edge]
    three = [base * 1.1, r_edge, base * 0.9]
    eight = [base, 1e30, 0.0, r_edge, 1e-3, base * 0.8, float(np.nextafter(np.float32(r_edge), np.float32(4))), base * 1.3]
    nine = eight + [base * 1.05]
    infos = {}
    for radii in (one, three, eight, nine):
        info = infos[len(radii)] = check_pops(dens, Q, R, d2, radii, what="boundary")
        assert info[2] > 0, "pairs exactly on a radius can only be decided by the exact path"
        want = expect_pops(d2, radii)
        k = radii.index(r_edge)
        for a, b, c, d in groups:
            assert want[k][a] >= 1   # (the pair one ulp inside the radius counts, the one on it does not)
    want = expect_pops(d2, eight)
    assert (want[eight.index(1e30)] == len(R)).all() and (want[eight.index(0.0)] == 0).all(), "no self term: radius 0 holds nothing"
    # 300 x 300: 3 x 3 blocks of 16 tile pairs, 16 MFMAs per tile pair at 80 columns; nine radii are two launches
    assert infos[8][:2] == (144, 144 * 16) and infos[9][:2] == (2 * 144, 2 * 144 * 16)


def test_ties_and_duplicates_the_lowest_index_wins(dens):
    Q, R, stars, copies, twins = cw.ties_sets(130, 200, 129)
    d2 = block_d2(the_probe(), Q, R)
    fe_q, fe_r = cw.fe_pair(len(Q), len(R))
    check_pops(dens, Q, R, d2, cw.radii_for(129, 3) + [2.0 ** -6, float(np.nextafter(np.float32(2.0 ** -6), np.float32(1)))])
    check_nn(dens, Q, R, d2, fe_q, fe_r)
    got = dens.nearest_reference_wide(gpu(Q), gpu(R))
    idx, dd = host(got[0]), host(got[1])
    for q, ring in stars:
        assert idx[q] == min(ring) and dd[q] == np.float32(2.0 ** -12)
    for q, j in copies:
        assert idx[q] == j and dd[q] == 0
    for q, lo, hi in twins:
        assert idx[q] == lo and dd[q] == 0


@pytest.mark.parametrize("n_rows,n_cols", [(300, 100), (1100, 65)])
def test_queries_and_reference_in_the_same_array(dens, n_rows, n_cols):
    """Q == R, the same pointer: an ordinary pair of sets -- every frame meets itself"""
    import torch
    c = wideref.blobs(n_rows, n_cols)
    d2 = block_d2(the_probe(), c, c)
    ct = torch.from_numpy(c).cuda()
    radii = cw.radii_for(n_cols, 3)
    got = dens.calculate_populations_against_wide(ct, ct, radii)
    answered(dens, ct.device, n_cols, "Q == R", cw.tile_pairs(n_rows, n_rows))
    same_pops(got, expect_pops(d2, radii), "Q == R")
    self_pops = dens.calculate_populations_wide(ct, radii)
    assert bool((got == self_pops).all()), "for r > 0 the pair (i, i) is the self sweep's own 1"
    fe = dens.calculate_free_energies(self_pops[0].contiguous())
    nn = dens.nearest_reference_wide(ct, ct, fe, fe)
    answered(dens, ct.device, n_cols, "Q == R neighbours", cw.tile_pairs(n_rows, n_rows))
    feh = host(fe)
    same_nn(nn, expect_nn(d2, feh, feh), "Q == R")
    assert bool((nn[0] == torch.arange(n_rows, device="cuda", dtype=torch.int32)).all()) and bool((nn[1] == 0).all())
    self_nn = dens.nearest_neighbors_wide(ct, fe)
    assert bool((nn[2] == self_nn[2]).all()) and bool((nn[3].view(torch.int32) == self_nn[3].view(torch.int32)).all()), \
        "a frame is not lower than itself: nn_hd is the self sweep's"


def test_free_energies_of_any_kind_on_both_sides(dens):
    Q, R, d2 = sets_case(129, 130, 200)
    fams_q, fams_r = wideref.fe_families(len(Q)), wideref.fe_families(len(R))
    for kq, fq in fams_q.items():
        for kr, fr in fams_r.items():
            check_nn(dens, Q, R, d2, fq, fr, what=(kq, kr))
    _, fr = cw.fe_pair(len(Q), len(R))
    lowest = expect_nn(d2, np.full(len(Q), -np.inf, dtype=np.float32), fr)
    assert (lowest[2] == len(R) + 1).all() and (lowest[3] == FLT_MAX).all(), "nothing lies below -inf"
    check_nn(dens, Q, R, d2, np.full(len(Q), -np.inf, dtype=np.float32), fr, what="fe_query -inf")
    highest = expect_nn(d2, np.full(len(Q), np.inf, dtype=np.float32), fr)
    assert (highest[2] == highest[0]).all(), "everything finite lies below +inf: nn_hd is nn"
    check_nn(dens, Q, R, d2, np.full(len(Q), np.inf, dtype=np.float32), fr, what="fe_query +inf")
    # no free energies: nn alone, unchanged, and no hd output
    check_nn(dens, Q, R, d2, None, None, what="nn only")


@pytest.mark.parametrize("side", ["query", "reference", "both"])
def test_nan_free_energies_results_only(dens, side):
    Q, R, d2 = sets_case(129, 130, 200)
    fq, fr = cw.fe_pair(len(Q), len(R))
    if side in ("query", "both"):
        fq[[0, 37, 129]] = np.nan
    if side in ("reference", "both"):
        fr[[1, 64, 199]] = np.nan
    check_nn(dens, Q, R, d2, fq, fr, finite=False, what=("NaN fe", side))


@pytest.mark.parametrize("what", ["scale 1e-6", "scale 1e6", "offset 1e3", "queries a blob distance away"])
def test_scaled_and_offset_data(dens, what):
    radii = cw.radii_for(100, 3)
    if what == "queries a blob distance away":
        Q, R = cw.offset_sets(100, 130, 200)
    else:
        Q, R = cw.blob_sets(100, 130, 200)
        if what == "offset 1e3":
            Q, R = (Q + np.float32(1000.0)).astype(np.float32), (R + np.float32(1000.0)).astype(np.float32)
        else:
            f = np.float32(1e-6 if what == "scale 1e-6" else 1e6)
            Q, R, radii = (Q * f).astype(np.float32), (R * f).astype(np.float32), [float(np.float32(r) * f) for r in radii]
    Q, R = np.ascontiguousarray(Q), np.ascontiguousarray(R)
    d2 = block_d2(the_probe(), Q, R)
    check_both(dens, Q, R, d2, radii, what=what)
    if what == "queries a blob distance away":
        assert int(expect_pops(d2, radii).sum()) == 0


@pytest.mark.parametrize("flaw", cw.FLAWS)
def test_flagged_data_is_answered_by_the_direct_kernels(dens, flaw):
    import torch
    Q0, R0 = cw.blob_sets(100, 130, 200)
    Q, R = cw.flawed_sets(Q0, R0, flaw)
    assert crossref.stats_flagged(Q, R)
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = block_d2(the_probe(), Q, R)
    radii = cw.radii_for(100, 3)
    fq, fr = cw.fe_pair(len(Q), len(R))
    q, r, fqt, frt = gpu(Q), gpu(R), gpu(fq), gpu(fr)
    got = dens.calculate_populations_against_wide(q, r, radii)
    assert dens.wide_against_info(q.device) == (0, 0, 0)
    assert bool((got == dens.calculate_populations_against(q, r, radii, variant="direct")).all())
    same_pops(got, expect_pops(d2, radii), flaw)
    nn = dens.nearest_reference_wide(q, r, fqt, frt, 10, 120)
    assert dens.wide_against_info(q.device) == (0, 0, 0)
    for x, y in zip(nn, dens.nearest_reference(q, r, fqt, frt, 10, 120, variant="direct")):
        assert bool((x.view(torch.int32) == y.view(torch.int32)).all())
    same_nn(nn, expect_nn(d2, fq, fr, 10, 120), flaw)
    row = cw.flawed_row(Q, R, flaw)
    if not flaw.startswith("big"):
        if flaw.endswith("query"):
            assert int(got[:, row].sum()) == 0 and int(nn[0][row]) == len(R) + 1, "a non-finite query has no partners and no neighbour"
        else:
            assert not bool((nn[0] == row).any()) and not bool((nn[2] == row).any()), "a non-finite reference is never a neighbour"
    # ... and the next call on clean data in the same workspace runs on the matrix cores again
    check_pops(dens, Q0, R0, block_d2(the_probe(), Q0, R0), radii)


def test_both_sweeps_in_one_workspace_in_either_order(dens):
    import torch
    from clustering_amd import capi
    big = sets_case(100, 300, 200)
    small = sets_case(100, 33, 127)
    radii = cw.radii_for(100, 3)
    rad = np.ascontiguousarray(radii, dtype=np.float32)
    need = capi.lib.dc_hip_cross_wide_workspace_bytes(300, 200, 100, len(radii))
    assert need >= capi.lib.dc_hip_cross_wide_workspace_bytes(33, 127, 100, len(radii))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    c_self = torch.from_numpy(wideref.blobs(200, 100)).cuda()

    def info():
        t, m, e = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        capi.check(capi.lib.dc_hip_wide_info_dev(p(ws), C.byref(t), C.byref(m), C.byref(e), None))
        return t.value, m.value, e.value

    def populations(case):
        Q, R, d2 = case
        q, r = gpu(Q), gpu(R)
        out = torch.full((len(radii), len(Q)), -1, dtype=torch.int32, device="cuda")
        capi.check(capi.lib.dc_hip_populations_cross_wide_dev(p(q), len(Q), p(r), len(R), 100, rad.ctypes.data_as(C.POINTER(C.c_float)),
                                                              len(radii), 0, len(Q), p(out), p(ws), need, None))
        torch.cuda.synchronize()
        same_pops(out, expect_pops(d2, radii), "one workspace")
        assert info()[:2] == (cw.tile_pairs(len(Q), len(R)), 19 * cw.tile_pairs(len(Q), len(R)))

    def neighbours(case):
        Q, R, d2 = case
        q, r = gpu(Q), gpu(R)
        fq, fr = cw.fe_pair(len(Q), len(R))
        fqt, frt = gpu(fq), gpu(fr)
        o = [torch.full((len(Q),), -1, dtype=torch.int32, device="cuda"), torch.full((len(Q),), -1.0, device="cuda"),
             torch.full((len(Q),), -1, dtype=torch.int32, device="cuda"), torch.full((len(Q),), -1.0, device="cuda")]
        capi.check(capi.lib.dc_hip_nearest_neighbors_cross_wide_dev(p(q), len(Q), p(r), len(R), 100, p(fqt), p(frt), 0, len(Q),
                                                                    p(o[0]), p(o[1]), p(o[2]), p(o[3]), p(ws), need, None))
        torch.cuda.synchronize()
        same_nn(o, expect_nn(d2, fq, fr), "one workspace")
        t, m, e = info()
        assert (t, m) == (cw.tile_pairs(len(Q), len(R)), 19 * cw.tile_pairs(len(Q), len(R))) and e > 0

    def self_sweep(_):
        # the wide self sweeps keep a cache of their own: neither disturbs the other
        before = dens.wide_against_info("cuda:0")
        dens.calculate_populations_wide(c_self, radii)
        assert dens.wide_sweep_info(c_self.device)[0] == 16 * 2 * 2
        assert dens.wide_against_info("cuda:0") == before

    for order in ((populations, neighbours, populations), (neighbours, populations, neighbours)):
        for case in (big, small, big):
            for k, call in enumerate(order):
                call(case)
                if k == 0:
                    self_sweep(case)
    # through the Python cache: a self call between two cross calls changes the counters of neither
    Q, R, d2 = small
    check_pops(dens, Q, R, d2, radii)
    self_sweep(None)
    check_nn(dens, Q, R, d2, *cw.fe_pair(len(Q), len(R)))


def test_assign_frames_wide_end_to_end(dens):
    import torch
    n_q, n_r, D = 200, 600, 100
    Q, R = crossref.sets(D, n_q, n_r, seed=41)
    probe = the_probe()
    radius = crossref.radius(D)
    states_r = (np.arange(n_r) % 5 + 1).astype(np.int32)
    q, r = gpu(Q), gpu(R)
    got = dens.assign_frames_wide(q, r, radius, states_r)
    assert dens.wide_against_info(q.device)[0] == cw.tile_pairs(n_q, n_r) and dens.wide_sweep_info(q.device)[0] == cw.tile_pairs(n_r, n_r)
    # the restatement from the probe: the reference's own populations carry the frame itself (d2 = 0 < r^2)
    d2_rr, d2_qr = block_d2(probe, R, R), block_d2(probe, Q, R)
    pops_ref = expect_pops(d2_rr, [radius])[0]
    max_pop = int(pops_ref.max())
    fe_ref = crossref.fe_of(pops_ref, max_pop)
    pops_q = expect_pops(d2_qr, [radius])[0]
    fe_q = crossref.fe_of(pops_q, max_pop)
    nn_i, nn_d, hd_i, hd_d = expect_nn(d2_qr, fe_q, fe_ref)
    pick = np.where(hd_i != n_r + 1, hd_i, nn_i)
    states = np.where(pick != n_r + 1, states_r[np.minimum(pick, n_r - 1)], 0)
    assert (host(got["pops_ref"]) == pops_ref).all() and got["max_pop"] == max_pop
    assert (bits(host(got["fe_ref"])) == bits(fe_ref)).all()
    assert (host(got["pops"]) == pops_q).all() and (bits(host(got["fe"])) == bits(fe_q)).all()
    same_nn((got["nn_idx"], got["nn_d2"], got["hd_idx"], got["hd_d2"]), [nn_i, nn_d, hd_i, hd_d], "assign_frames_wide")
    assert (host(got["states"]) == states).all() and int((states == 0).sum()) == 0
    # ... and assign_frames on the direct kernels, key by key
    ref = dens.assign_frames(q, r, radius, states_r, variant="direct")
    assert set(got) == set(ref)
    for key, val in ref.items():
        if key == "max_pop":
            assert got[key] == val
        else:
            assert got[key].dtype == val.dtype and got[key].shape == val.shape, key
            assert bool((got[key].view(torch.int32) == val.view(torch.int32)).all()), key


CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from clustering_amd import capi, density as dens
from oracle.oracle import Probe
import crossref, crosswideref as cw
ORDER = sys.argv[2]
assert capi.lib.dc_hip_canon_order().decode() == ORDER
probe = Probe(ORDER)
for n_q, n_r, d in ((130, 200, 65), (300, 300, 100), (97, 161, 129), (130, 200, 256)):
    for (Q, R), radii in ((cw.ties_sets(n_q, n_r, d)[:2], cw.radii_for(d, 3)),
                          (cw.boundary_sets(n_q, n_r, d)[:2], [cw.BOUNDARY_RADIUS, float(np.sqrt(0.18 * d))])):
        d2 = crossref.block_d2(probe, Q, R)
        q, r = crossref.gpu(Q), crossref.gpu(R)
        got = dens.calculate_populations_against_wide(q, r, radii)
        t, m, e = dens.wide_against_info(q.device)
        assert t == cw.tile_pairs(n_q, n_r) and m == cw.nm_for(d) * t, (n_q, n_r, d, t, m)
        assert (crossref.host(got) == crossref.expect_pops(d2, radii)).all(), (n_q, n_r, d, "pops")
        fq, fr = cw.fe_pair(n_q, n_r)
        g = dens.nearest_reference_wide(q, r, crossref.gpu(fq), crossref.gpu(fr))
        assert dens.wide_against_info(q.device)[0] == cw.tile_pairs(n_q, n_r)
        crossref.same_nn(g, crossref.expect_nn(d2, fq, fr), (n_q, n_r, d))
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


@pytest.mark.parametrize("n_cols", [65, 256])
def test_blob_sets_send_at_most_one_percent_to_the_exact_path(dens, n_cols):
    """the cap the self sweeps are held to (tests/test_gpu_wide_mfma.py), on sets without the injected duplicates of
    crossref.sets: a duplicate pair is a legitimate candidate"""
    Q, R = cw.blob_sets(n_cols, 1500, 1500)
    d2 = block_d2(the_probe(), Q, R)
    radii = [float(np.sqrt(np.quantile(d2, 0.25))), float(np.sqrt(np.quantile(d2, 0.05)))]
    tiles, mfmas, exact = check_pops(dens, Q, R, d2, radii)
    print(f"D={n_cols}: {tiles} tile pairs, {mfmas} MFMAs, {exact} exact pairs = {100.0 * exact / (1024 * tiles):.4f} % of the evaluated pairs")
    assert exact <= 0.01 * 1024 * tiles
    fe_r = crossref.fe_of(expect_pops(block_d2(the_probe(), R, R), radii[:1])[0], 1500)
    fe_q = crossref.fe_of(expect_pops(d2, radii[:1])[0], 1500)
    tiles, mfmas, exact = check_nn(dens, Q, R, d2, fe_q, fe_r)
    print(f"D={n_cols} neighbours: {exact} exact pairs = {100.0 * exact / (1024 * tiles):.4f} % of the evaluated pairs")
    assert exact <= 0.01 * 1024 * tiles, "the neighbour sweep's candidates: the same cap"
