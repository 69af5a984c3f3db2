"""GPU (-m gpu): the pruned matrix-core population sweep of new frames against a reference
(calculate_populations_against(..., variant="cross_pruned"), DC_VARIANT_CROSS_PRUNED) against the probe's canonical d2
(crossref.block_d2 / expect_pops): every width, who answered, exact radius boundaries, special radii, degenerate grids,
flagged data, refusals, assign_frames, and the libraries of the other summation orders.  The premises of the built
cases are checked without a GPU in tests/test_cross_pruned_cases.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import crossprunedref as cp
from crossref import F32, block_d2, expect_pops, gpu, host, radius, sets
from clustering_amd.synth import gaussian_blobs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = "cross_pruned"


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


def tiles(n):
    return (n + 31) // 32


def check(dens, probe, Q, R, radii, what, i_from=0, i_to=None):
    d2 = block_d2(probe, Q, R)
    exp = expect_pops(d2, radii, i_from, i_to)
    got = host(dens.calculate_populations_against(gpu(Q), gpu(R), radii, i_from, len(Q) if i_to is None else i_to, variant=V))
    bad = np.argwhere(got != exp)
    assert bad.size == 0, (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])
    return exp


# ---- 1 --------------------------------------------------------------------------------------------------------------
WIDTHS = [1, 2, 3, 4, 5, 9, 10, 16, 26, 27, 30, 33, 64]   # both sides of every step of TQ (NM 2|3, 5|6) and of NM
SHAPES = [(1037, 2311), (1, 33), (33, 1), (31, 32), (32, 31), (33, 33)]


@pytest.mark.parametrize("D", WIDTHS)
def test_every_width(dens, probe, D):
    for n_q, n_r in SHAPES:
        Q, R = sets(D, n_q, n_r, seed=D * 7 + n_q)
        r0 = radius(D)
        i_from, i_to = n_q // 5, n_q - n_q // 7
        exp = check(dens, probe, Q, R, [r0, 0.5 * r0, 2.0 * r0], (D, n_q, n_r), i_from, i_to)
        assert (exp[:, :i_from] == 0).all() and (exp[:, i_to:] == 0).all()


# ---- 2 --------------------------------------------------------------------------------------------------------------
def test_who_answered(dens, probe):
    """The counters of the workspace say that the pruned sweep answered and that it pruned.
    The cap 0.75 T_q T_r is a condition, not a measurement: R is two blobs of 1024 frames = 32 tiles each in cell
    order, 100 apart, Q lies on the first.  A query tile can meet at most the tiles of its own blob plus one tile that
    straddles the two: 33 of 64.  The sweep counts whole query groups of up to 6 tiles: 32 query tiles are padded to
    at most 36, a factor 36 / 32.  Together at most 33 / 64 * 36 / 32 = 0.58 of T_q T_r."""
    import torch
    Q, R = cp.two_blobs()
    T_q, T_r = tiles(len(Q)), tiles(len(R))
    exp = check(dens, probe, Q, R, [cp.BLOB_R], "two blobs")
    assert exp.max() > 0
    pop_tiles, pop_mfma = dens.evaluated_tiles_against(torch.device("cuda", torch.cuda.current_device()))
    print("two blobs: pop_tiles", pop_tiles, "of", T_q * T_r, "pop_mfma", pop_mfma)
    assert 0 < pop_tiles <= 0.75 * T_q * T_r, (pop_tiles, T_q * T_r)
    assert pop_mfma > 0
    # between the blobs, more than r from both in column 0: nothing survives the box test
    exp = check(dens, probe, cp.shifted(Q), R, [cp.BLOB_R], "between the blobs")
    assert (exp == 0).all()
    pop_tiles, pop_mfma = dens.evaluated_tiles_against(torch.device("cuda", torch.cuda.current_device()))
    assert pop_tiles == 0 and pop_mfma == 0, (pop_tiles, pop_mfma)


# ---- 3 --------------------------------------------------------------------------------------------------------------
def lattice_programme(dens, probe, D):
    g, (r_at, r_above, r_below) = cp.lattice_radii()
    for Q, R in (cp.lattice_sets(D, g), cp.lattice_gap_sets(D, g)):
        for radii in ([r_at], [r_above], [r_below], [r_above, r_below, r_at]):
            exp = check(dens, probe, Q, R, radii, ("lattice", D, len(Q), radii))
        assert (exp[0] > exp[2]).any() and (exp[1] == exp[2]).all()   # strict '<' on both sides of the ties


@pytest.mark.parametrize("D", [2, 3, 10])
def test_boundary_lattice(dens, probe, D):
    lattice_programme(dens, probe, D)


# ---- 4 --------------------------------------------------------------------------------------------------------------
def test_special_radii(dens, probe):
    """0, a negative radius, NaN, a radius whose square is +inf and an ordinary one in one call.  fl32(1e20^2) = inf:
    every finite pair is inside and nothing may be pruned -- the pruned sweep answers that radius itself (gap < inf
    holds for every pair of real tiles), so its counter holds at least T_q T_r tile pairs after the call."""
    import torch
    D, n_q, n_r = 10, 300, 500
    Q, R = sets(D, n_q, n_r, seed=4)
    r0 = radius(D)
    exp = check(dens, probe, Q, R, [0.0, -1.0, float("nan"), 1e20, r0], "special radii")
    assert (exp[0] == 0).all() and (exp[2] == 0).all() and (exp[3] == n_r).all() and (exp[1] >= exp[4]).all()
    pop_tiles, _ = dens.evaluated_tiles_against(torch.device("cuda", torch.cuda.current_device()))
    assert pop_tiles >= tiles(n_q) * tiles(n_r), pop_tiles


# ---- 5, 6 -----------------------------------------------------------------------------------------------------------
def test_same_buffer_on_both_sides_keeps_the_self_pair(dens, probe):
    D, n = 10, 777
    c = gaussian_blobs(n, D, seed=D + 17)
    rng = np.random.default_rng(D)
    c[rng.integers(0, n, n // 8)] = c[rng.integers(0, n, n // 8)]   # exact copies, before and after their originals
    radii = [0.0, radius(D), 0.5 * radius(D)]
    exp = expect_pops(block_d2(probe, c, c), radii)
    assert (exp[0] == 0).all() and (exp[1] >= 1).all() and (exp[2] >= 1).all()
    t = gpu(c)
    assert (host(dens.calculate_populations_against(t, t, radii, variant=V)) == exp).all()


def test_query_equals_reference_gives_the_self_populations(dens, oracle):
    c = gaussian_blobs(20000, 10, seed=3)
    radii = [0.2, 0.1, 0.3]
    want = oracle.populations(c, radii)
    t = gpu(c)
    got = dens.calculate_populations_against(t, t, radii, variant=V)
    assert (host(got).astype(np.uint64) == want).all()


# ---- 7 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [3, 10, 30])
def test_scale_edges(dens, probe, D):
    rng = np.random.default_rng(D)
    R = (rng.normal(size=(1500, D)) * 0.02).astype(np.float32)
    Q = (R[:700] + F32(1e4)).astype(np.float32)
    Q[::7] = R[:700:7] + (rng.normal(size=(100, D)) * 0.01).astype(np.float32)
    check(dens, probe, Q, R, [0.05, 0.02, 0.1], "offset 1e4")
    Q = (rng.normal(size=(500, D)) * 0.02 + 1000.0).astype(np.float32)
    assert (check(dens, probe, Q, R, [0.5], "far away") == 0).all()
    tiny = (rng.normal(size=(900, D)) * 1e-3).astype(np.float32)
    large = (rng.normal(size=(800, D)) * 50.0).astype(np.float32)
    large[::5] = tiny[:160] * F32(3.0)
    check(dens, probe, large, tiny, [0.003, 1e-3, 30.0], "tiny reference")
    check(dens, probe, tiny, large, [0.003, 1e-3, 30.0], "tiny queries")
    R2 = np.repeat(gaussian_blobs(400, D, seed=D), 3, axis=0)[np.random.default_rng(1).permutation(1200)]
    check(dens, probe, R2[::5].copy(), R2, [radius(D)], "duplicates")


# ---- 8 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 10])
def test_non_finite_rows_and_an_empty_reference(dens, probe, D):
    Q, R = sets(D, 700, 900, seed=D)
    clean = (Q.copy(), R.copy())
    Q[3, 0] = np.inf
    Q[10, D - 1] = np.nan
    R[5, 0] = -np.inf
    R[17, D // 2] = np.nan
    exp = check(dens, probe, Q, R, [radius(D), 2 * radius(D)], "non-finite")
    assert (exp[:, [3, 10]] == 0).all()
    check(dens, probe, clean[0], clean[1], [radius(D), 2 * radius(D)], "clean, after a flagged call in the same workspace")
    empty = gpu(np.zeros((0, D), np.float32))
    assert (host(dens.calculate_populations_against(gpu(Q), empty, [1.0, 2.0], variant=V)) == 0).all()


# ---- 9 --------------------------------------------------------------------------------------------------------------
def test_degenerate_grids(dens, probe):
    for name, Q, R, radii in cp.degenerate_cases():
        exp = check(dens, probe, Q, R, radii, name)
        assert exp.max() > 0, name


# ---- 10 -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_next_call_right(dens, probe):
    import torch
    from clustering_amd import capi
    Q, R = sets(65, 100, 200, seed=1)
    with pytest.raises(RuntimeError):
        dens.calculate_populations_against(gpu(Q), gpu(R), [1.0], variant=V)
    Q, R = sets(10, 300, 700, seed=2)
    q, r = gpu(Q), gpu(R)
    with pytest.raises(RuntimeError):
        dens.nearest_reference(q, r, variant=V)
    # a workspace one byte short: DC_ERR_WORKSPACE (-5 in include/dc_density.h), straight from the C ABI
    need = capi.lib.dc_hip_cross_workspace_bytes_for(300, 700, 10, capi.VARIANT_CROSS_PRUNED)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.zeros((1, 300), dtype=torch.int32, device="cuda")
    rad = (ctypes.c_float * 1)(0.2)
    args = (ctypes.c_void_p(q.data_ptr()), 300, ctypes.c_void_p(r.data_ptr()), 700, 10, rad, 1, 0, 300,
            ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert capi.lib.dc_hip_populations_cross_dev(*args, need - 1, capi.VARIANT_CROSS_PRUNED, stream) == -5
    assert capi.lib.dc_hip_populations_cross_dev(*args, need, capi.VARIANT_CROSS_PRUNED, stream) == 0
    exp = expect_pops(block_d2(probe, Q, R), [0.2])
    assert (host(out) == exp).all()
    check(dens, probe, Q, R, [0.2, 0.1], "after the refusals")


# ---- 11 -------------------------------------------------------------------------------------------------------------
def test_assign_frames(dens):
    c = gaussian_blobs(7000, 10, seed=8)
    q, r = gpu(c[:2000]), gpu(c[2000:])
    states = (np.arange(5000) % 7 + 1).astype(np.int32)
    want = dens.assign_frames(q, r, 0.2, states, variant="direct")
    got = dens.assign_frames(q, r, 0.2, states, variant=V)
    for k in want:
        a, b = want[k], got[k]
        if isinstance(a, int):
            assert a == b, k
        else:
            assert (host(a).view(np.uint32) == host(b).view(np.uint32)).all(), k


# ---- 12 -------------------------------------------------------------------------------------------------------------
CHILD = r"""
import os, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from clustering_amd import capi, density as dens
from oracle.oracle import Probe
import test_gpu_cross_pruned as t
assert capi.lib.dc_hip_canon_order().decode() == sys.argv[2] == capi.CANON_ORDER
t.lattice_programme(dens, Probe(capi.CANON_ORDER), 10)
print("ok")
"""


@pytest.mark.parametrize("order", ["avx", "fma"])
def test_other_order_libraries(order):
    """the boundary lattice at D = 10 on the library of another summation order, in a fresh child process"""
    if not os.path.exists(os.path.join(ROOT, "clustering_amd", "lib_" + order, "libdcdensity.so")):
        pytest.fail(f"clustering_amd/lib_{order}/libdcdensity.so is missing: __graft_entry__.build() makes it")
    env = dict(os.environ, DC_CANON_ORDER=order)
    env.pop("DC_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, order], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
