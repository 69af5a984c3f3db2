"""GPU: the matrix-core sweeps for rows of 65..256 columns (density.calculate_populations_wide / nearest_neighbors_wide)
against the CPU oracle, bit for bit: populations, nn_idx, nn_d2 bits, hd_idx, hd_d2 bits.  Every finite case first asserts
that the matrix-core kernel answered (wide_sweep_info: tiles > 0) -- a silent fall-back to the direct kernels would
otherwise pass.  Cases: tests/wideref.py (their conditions are checked on the CPU by tests/test_wide_mfma_cases.py)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import wideref

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


def radii_for(n_cols, k=3):
    """k radii around the intra-blob distance of synth.gaussian_blobs (d2 ~ 2 sigma^2 D), not sorted"""
    base = float(np.sqrt(2 * 0.08 * 0.08 * n_cols))
    return [base * f for f in (1.0, 0.9, 1.08, 0.95, 1.2, 0.8, 1.02, 0.85)[:k]]


@functools.lru_cache(maxsize=None)
def blob_reference(n_rows, n_cols, k):
    """(coords, radii, populations, free energies of the first radius, neighbours): computed once per shape"""
    from oracle.oracle import Oracle
    o = Oracle()
    c = wideref.blobs(n_rows, n_cols)
    radii = radii_for(n_cols, k)
    pops = o.populations(c, radii)
    fe = o.free_energies(pops[0])
    return c, radii, pops, fe, o.nearest_neighbors(c, fe)


def check_pops(dens, oracle, c, radii, lo=0, hi=None, want=None, finite=True):
    import torch
    hi = len(c) if hi is None else hi
    ct = torch.from_numpy(c).cuda()
    got = dens.calculate_populations_wide(ct, radii, lo, hi)
    info = dens.wide_sweep_info(ct.device)
    if finite and hi > lo:
        assert info[0] > 0 and info[1] > 0, "the matrix-core kernel did not answer"
    if want is None:
        want = oracle.populations(c, radii, lo, hi)
    assert (u64(got) == want).all(), ("populations", c.shape, radii, lo, hi)
    return info


def check_nn(dens, oracle, c, fe, lo=0, hi=None, want=None, finite=True):
    import torch
    hi = len(c) if hi is None else hi
    ct = torch.from_numpy(c).cuda()
    got = dens.nearest_neighbors_wide(ct, torch.from_numpy(np.ascontiguousarray(fe, dtype=np.float32)).cuda(), lo, hi)
    info = dens.wide_sweep_info(ct.device)
    if finite and hi > lo:
        assert info[0] > 0 and info[1] > 0, "the matrix-core kernel did not answer"
    if want is None:
        want = oracle.nearest_neighbors(c, fe, lo, hi)
    assert (u64(got[0]) == want[0]).all(), ("nn_idx", c.shape, lo, hi)
    assert (bits(got[1].cpu().numpy()) == bits(want[1])).all(), ("nn_d2", c.shape, lo, hi)
    assert (u64(got[2]) == want[2]).all(), ("hd_idx", c.shape, lo, hi)
    assert (bits(got[3].cpu().numpy()) == bits(want[3])).all(), ("hd_d2", c.shape, lo, hi)
    return info


@pytest.mark.parametrize("n_cols", wideref.COLS)
def test_column_counts_on_both_sides_of_every_seam(dens, oracle, n_cols):
    c, radii, pops, fe, nn = blob_reference(200, n_cols, 3)
    check_pops(dens, oracle, c, radii, want=pops)
    check_nn(dens, oracle, c, fe, want=nn)


@pytest.mark.parametrize("n_rows", wideref.ROWS)
def test_row_counts_from_one_frame_to_several_workgroups(dens, oracle, n_rows):
    c, radii, pops, fe, nn = blob_reference(n_rows, 100, 1)
    info = check_pops(dens, oracle, c, radii, want=pops)
    assert info[1] == 19 * info[0], "19 MFMAs per tile pair at 100 columns"
    check_nn(dens, oracle, c, fe, want=nn)
    if n_rows == 1:
        assert int(pops[0][0]) == 1 and int(nn[0][0]) == 2 and nn[1][0] == FLT_MAX


@pytest.mark.parametrize("lo,hi", [(37, 171), (128, 256), (0, 1), (299, 300), (33, 290), (5, 5), (300, 300)])
def test_row_ranges_that_start_and_end_inside_tiles(dens, oracle, lo, hi):
    c, radii, _, fe, _ = blob_reference(300, 100, 3)
    info_p = check_pops(dens, oracle, c, radii, lo, hi)
    info_n = check_nn(dens, oracle, c, fe, lo, hi)
    if lo == hi:
        assert info_p == (0, 0, 0) and info_n == (0, 0, 0), "nothing swept: zeros / none, and counters that say so"


def test_radii_in_any_order_and_at_the_edges(dens, oracle):
    c, r_edge, groups = wideref.boundary_case(300, 80)
    base = float(np.sqrt(2 * 0.3 * 0.3 * 80))
    one = [r_edge]
    three = [base * 1.1, r_edge, base * 0.9]
    eight = [base, 1e30, 0.0, r_edge, 1e-3, base * 0.8, float(np.nextafter(np.float32(r_edge), np.float32(4))), base * 1.3]
    for radii in (one, three, eight):
        want = oracle.populations(c, radii)
        info = check_pops(dens, oracle, c, radii, want=want)
        assert info[2] > 0, "pairs exactly on a radius can only be decided by the exact path"
        k = radii.index(r_edge)
        for a, b, cc, d in groups:
            inside = int(want[k][a])
            assert inside >= 2   # (the pair one ulp inside the radius counts, the one on it does not)
    big, zero, tiny = eight.index(1e30), eight.index(0.0), eight.index(1e-3)
    want = oracle.populations(c, eight)
    assert (want[big] == len(c)).all() and (want[zero] == 1).all()
    assert int(want[tiny].max()) <= 4   # (only the rows the groups copied)
    # more radii than one launch takes: two launches, and the counters cover both (300 rows: 3 x 3 blocks of 16 tile pairs)
    info8 = check_pops(dens, oracle, c, eight, want=want)
    eleven = eight + [base * 1.05, base * 0.7, r_edge]
    info11 = check_pops(dens, oracle, c, eleven)
    assert info8[:2] == (144, 144 * 16) and info11[:2] == (2 * 144, 2 * 144 * 16), "16 MFMAs per tile pair at 80 columns"


@pytest.mark.parametrize("n_cols", [65, 256])
def test_blob_case_sends_at_most_one_percent_to_the_exact_path(dens, oracle, n_cols):
    c = wideref.blobs(1500, n_cols)
    x = c.astype(np.float64)
    g = (x * x).sum(axis=1)
    d2 = np.maximum(g[:, None] + g[None, :] - 2.0 * (x @ x.T), 0.0)
    off = d2[~np.eye(len(c), dtype=bool)]
    radii = [float(np.sqrt(np.quantile(off, 0.25))), float(np.sqrt(np.quantile(off, 0.05)))]
    tiles, mfmas, exact = check_pops(dens, oracle, c, radii)
    print(f"D={n_cols}: {tiles} tile pairs, {mfmas} MFMAs, {exact} exact pairs = {100.0 * exact / (1024 * tiles):.4f} % of the evaluated pairs")
    assert exact <= 0.01 * 1024 * tiles
    pops = oracle.populations(c, radii[:1])
    fe = oracle.free_energies(pops[0])
    tiles, mfmas, exact = check_nn(dens, oracle, c, fe)
    print(f"D={n_cols} neighbours: {exact} exact pairs = {100.0 * exact / (1024 * tiles):.4f} % of the evaluated pairs")
    assert exact <= 0.01 * 1024 * tiles, "the neighbour sweep's candidates: the same cap"


@pytest.mark.parametrize("what", ["scale 1e-6", "scale 1e6", "offset 1e3"])
def test_scaled_and_offset_data(dens, oracle, what):
    c, radii, _, _, _ = blob_reference(300, 100, 3)
    if what == "offset 1e3":
        c2, r2 = (c + np.float32(1000.0)).astype(np.float32), radii
    else:
        f = np.float32(1e-6 if what == "scale 1e-6" else 1e6)
        c2, r2 = (c * f).astype(np.float32), [float(np.float32(r) * f) for r in radii]
    c2 = np.ascontiguousarray(c2)
    pops = oracle.populations(c2, r2)
    check_pops(dens, oracle, c2, r2, want=pops)
    check_nn(dens, oracle, c2, oracle.free_energies(pops[0]))


@pytest.mark.parametrize("family", ["equal", "ties", "zeros", "populations"])
def test_free_energies_of_any_kind(dens, oracle, family):
    c, stars, dups = wideref.ties_case(300, 129)
    if family == "populations":
        fe = oracle.free_energies(oracle.populations(c, [radii_for(129, 1)[0]])[0])
    else:
        fe = wideref.fe_families(len(c))[family]
    want = oracle.nearest_neighbors(c, fe)
    check_nn(dens, oracle, c, fe, want=want)
    for q, ring in stars:
        assert int(want[0][q]) == min(ring)
    if family == "equal":
        assert (want[2] == len(c) + 1).all() and (want[3] == FLT_MAX).all(), "no frame of lower free energy anywhere"


@pytest.mark.parametrize("flaw", ["nan row", "inf row", "nan fe"])
def test_flagged_data_is_answered_by_the_direct_kernels(dens, oracle, flaw):
    import torch
    c, radii, pops, fe, _ = blob_reference(300, 100, 3)
    c, fe = c.copy(), fe.copy()
    if flaw == "nan row":
        c[131, 7] = np.nan
    elif flaw == "inf row":
        c[40, 99] = np.inf
    else:
        fe[77] = np.nan
    ct, ft = torch.from_numpy(c).cuda(), torch.from_numpy(fe).cuda()
    if flaw != "nan fe":
        got = dens.calculate_populations_wide(ct, radii)
        assert dens.wide_sweep_info(ct.device) == (0, 0, 0)
        assert bool((got == dens.calculate_populations_partial(ct, radii, variant="direct")).all())
    got = dens.nearest_neighbors_wide(ct, ft, 10, 290)
    assert dens.wide_sweep_info(ct.device) == (0, 0, 0)
    for x, y in zip(got, dens.nearest_neighbors_partial(ct, ft, 10, 290, variant="direct")):
        assert bool((x.view(torch.int32) == y.view(torch.int32)).all())
    # ... and the next call on clean data in the same workspace runs on the matrix cores again
    c, radii, pops, fe, nn = blob_reference(300, 100, 3)
    check_pops(dens, oracle, c, radii, want=pops)


def test_both_sweeps_in_one_workspace_in_either_order(dens, oracle):
    import ctypes as C
    import torch
    from clustering_amd import capi
    c, radii, pops, fe, nn = blob_reference(300, 100, 3)
    n, d = c.shape
    ct, ft = torch.from_numpy(c).cuda(), torch.from_numpy(fe).cuda()
    need = capi.lib.dc_hip_wide_workspace_bytes(n, d, len(radii))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rad = np.ascontiguousarray(radii, dtype=np.float32)
    p = lambda t: C.c_void_p(t.data_ptr())

    def populations():
        out = torch.full((len(radii), n), -1, dtype=torch.int32, device="cuda")
        capi.check(capi.lib.dc_hip_populations_wide_dev(p(ct), n, d, rad.ctypes.data_as(C.POINTER(C.c_float)), len(radii), 0, n,
                                                        p(out), p(ws), need, None))
        torch.cuda.synchronize()
        assert (u64(out) == pops).all()

    def neighbours():
        o = [torch.full((n,), -1, dtype=torch.int32, device="cuda"), torch.full((n,), -1.0, device="cuda"),
             torch.full((n,), -1, dtype=torch.int32, device="cuda"), torch.full((n,), -1.0, device="cuda")]
        capi.check(capi.lib.dc_hip_nearest_neighbors_wide_dev(p(ct), n, d, p(ft), 0, n, p(o[0]), p(o[1]), p(o[2]), p(o[3]),
                                                              p(ws), need, None))
        torch.cuda.synchronize()
        assert (u64(o[0]) == nn[0]).all() and (u64(o[2]) == nn[2]).all()
        assert (bits(o[1].cpu().numpy()) == bits(nn[1])).all() and (bits(o[3].cpu().numpy()) == bits(nn[3])).all()
        t, m, e = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        capi.check(capi.lib.dc_hip_wide_info_dev(p(ws), C.byref(t), C.byref(m), C.byref(e), None))
        assert t.value > 0 and m.value == 19 * t.value and e.value > 0

    for order in ((populations, neighbours), (neighbours, populations), (neighbours, neighbours, populations, populations)):
        for call in order:
            call()


CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from clustering_amd import capi, density as dens
from oracle.oracle import Oracle
import wideref
ORDER = sys.argv[2]
assert capi.lib.dc_hip_canon_order().decode() == ORDER
o = Oracle(order=ORDER)
bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
u64 = lambda t: t.cpu().numpy().astype(np.uint32).astype(np.uint64)
for n, d in ((200, 65), (300, 100), (97, 129), (200, 256)):
    for c, radii in ((wideref.ties_case(n, d)[0], [float(np.sqrt(0.0128 * d)) * f for f in (1.0, 0.9, 1.1)]),
                     (wideref.boundary_case(n, d)[0], [wideref.BOUNDARY_RADIUS, float(np.sqrt(0.18 * d))])):
        ct = torch.from_numpy(c).cuda()
        want = o.populations(c, radii)
        got = dens.calculate_populations_wide(ct, radii)
        assert dens.wide_sweep_info(ct.device)[0] > 0
        assert (u64(got) == want).all(), (n, d, "pops")
        fe = o.free_energies(want[0])
        exp = o.nearest_neighbors(c, fe)
        g = dens.nearest_neighbors_wide(ct, torch.from_numpy(fe).cuda())
        assert dens.wide_sweep_info(ct.device)[0] > 0
        assert (u64(g[0]) == exp[0]).all() and (u64(g[2]) == exp[2]).all(), (n, d, "nn idx")
        assert (bits(g[1].cpu().numpy()) == bits(exp[1])).all() and (bits(g[3].cpu().numpy()) == bits(exp[3])).all(), (n, d, "nn d2")
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
