"""GPU (-m gpu): the pruned matrix-core neighbour sweep of new frames against a reference
(nearest_reference(..., pruned=True), dc_hip_nearest_neighbors_cross_pruned_dev) against the probe's canonical d2
(crossref.block_d2 / expect_nn / same_nn: index and d2 bits equal): every width, who answered, ties across rings and
tiles, free energies of any origin, a lower frame only far away, identities, scale edges and degenerate grids,
non-finite rows, several shares, a reference beyond 2^24 positions, refusals, assign_frames, and the libraries of the
other summation orders.  The premises of the built cases are checked without a GPU in
tests/test_cross_nn_pruned_cases.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import crossnnref as cn
import crossprunedref as cp
import fe_families
from crossref import F32, FLT_MAX, block_d2, expect_nn, expect_pops, fe_of, gpu, host, radius, same_nn, sets
from clustering_amd.synth import gaussian_blobs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def info(dens):
    import torch
    return dens.evaluated_tiles_nearest_reference(torch.device("cuda", torch.cuda.current_device()))


def check(dens, probe, Q, R, fe_q, fe_r, what, i_from=0, i_to=None, d2=None):
    """with free energies (when given) and again with nn only"""
    d2 = block_d2(probe, Q, R) if d2 is None else d2
    i_to = len(Q) if i_to is None else i_to
    q, r = gpu(Q), gpu(R)
    if fe_q is not None:
        exp = expect_nn(d2, fe_q, fe_r, i_from, i_to)
        same_nn(dens.nearest_reference(q, r, gpu(fe_q), gpu(fe_r), i_from, i_to, pruned=True), exp, (what, "fe"))
    exp = expect_nn(d2, None, None, i_from, i_to)
    same_nn(dens.nearest_reference(q, r, None, None, i_from, i_to, pruned=True), exp, (what, "nn only"))
    return d2


def pipeline_fe(d2, probe, R, r0):
    """free energies of the real pipeline: fe_of on probe populations (the reference's self sweep has the self pair)"""
    pops_r = expect_pops(block_d2(probe, R, R), [r0])[0]
    pops_q = expect_pops(d2, [r0])[0]
    mx = int(pops_r.max())
    return fe_of(pops_q, mx), fe_of(pops_r, mx)


# ---- 1 --------------------------------------------------------------------------------------------------------------
WIDTHS = [1, 2, 3, 4, 5, 9, 10, 16, 26, 27, 30, 33, 64]   # both sides of every step of TQ (NM 2|3, 5|6) and of NM
SHAPES = [(1037, 2311), (1, 33), (33, 1), (31, 32), (32, 31), (33, 33)]


@pytest.mark.parametrize("D", WIDTHS)
def test_every_width(dens, probe, D):
    for n_q, n_r in SHAPES:
        Q, R = sets(D, n_q, n_r, seed=D * 7 + n_q)
        d2 = block_d2(probe, Q, R)
        fe_q, fe_r = pipeline_fe(d2, probe, R, radius(D))
        i_from, i_to = n_q // 5, n_q - n_q // 7
        check(dens, probe, Q, R, fe_q, fe_r, (D, n_q, n_r), i_from, i_to, d2=d2)
        exp = expect_nn(d2, fe_q, fe_r, i_from, i_to)
        assert (exp[0][:i_from] == n_r + 1).all() and (exp[1][i_to:] == FLT_MAX).all()


# ---- 2 --------------------------------------------------------------------------------------------------------------
def test_who_answered(dens, probe):
    """The counters say that the pruned kernel answered and that it pruned.  The cap 0.75 T_q T_r is a condition, not a
    measurement: R is two blobs of 32 tiles each in cell order, 100 apart, Q lies on the first, and every query has a
    lower-energy reference in its own blob so near that no ring reaches the other one (premise:
    test_cross_nn_pruned_cases.py).  A query tile can meet at most the 32 tiles of its blob plus one straddling tile:
    33 of 64.  The sweep counts whole query groups of TQ <= 6 tiles: 32 query tiles are padded to at most 36.  Together
    at most 33 / 64 * 36 / 32 = 0.58 of T_q T_r."""
    Q, R, fe_q, fe_r = cn.who_answered()
    T_q, T_r = tiles(len(Q)), tiles(len(R))
    d2 = block_d2(probe, Q, R)
    q, r, fq, fr = gpu(Q), gpu(R), gpu(fe_q), gpu(fe_r)
    same_nn(dens.nearest_reference(q, r, fq, fr, pruned=True), expect_nn(d2, fe_q, fe_r), "two blobs")
    nn_tiles, nn_mfma, n_shares = info(dens)
    print("two blobs: nn_tiles", nn_tiles, "of", T_q * T_r, "nn_mfma", nn_mfma, "shares", n_shares)
    assert 0 < nn_tiles <= 0.75 * T_q * T_r, (nn_tiles, T_q * T_r)
    assert nn_mfma > 0 and n_shares >= 1
    S = cp.shifted(Q)
    same_nn(dens.nearest_reference(gpu(S), r, fq, fr, pruned=True), expect_nn(block_d2(probe, S, R), fe_q, fe_r), "shifted")
    assert info(dens)[0] > 0
    # a flagged call: the direct kernel answers, all three counters are 0
    B = Q.copy()
    B[5, 1] = np.nan
    same_nn(dens.nearest_reference(gpu(B), r, fq, fr, pruned=True), expect_nn(block_d2(probe, B, R), fe_q, fe_r), "flagged")
    assert info(dens) == (0, 0, 0)


# ---- 3 --------------------------------------------------------------------------------------------------------------
def tie_programme(dens, probe, D):
    # (a) equal d2 in two reference tiles on opposite sides, the far one holding the lower indices and lying in the
    #     ring BEHIND the one whose end equals the incumbents (crossnnref.tie_sets; premise: test_tie_geometry)
    Q, R = cn.tie_sets(D)
    fe_q, fe_r = cn.tie_fe(len(Q), len(R))
    check(dens, probe, Q, R, fe_q, fe_r, ("tie tiles", D))
    # (b) shuffled overlapping lattices: several tiles, many cells, many equidistant candidates
    g, _ = cp.lattice_radii()
    Q, R = cp.lattice_sets(D, g)
    rng = np.random.default_rng(D)
    fe_r = (rng.integers(0, 5, len(R)) / 4.0).astype(np.float32)
    fe_q = (rng.integers(0, 6, len(Q)) / 4.0).astype(np.float32)
    check(dens, probe, Q, R, fe_q, fe_r, ("tie lattice", D))


@pytest.mark.parametrize("D", [2, 3, 10])
def test_ties_across_rings_and_tiles(dens, probe, D):
    tie_programme(dens, probe, D)


# ---- 4 --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fe_case(probe):
    Q, R = sets(10, 700, 1500, seed=44)
    return Q, R, block_d2(probe, Q, R)


@pytest.mark.parametrize("family", ["ties_ulp", "constant_3_5", "signed_zero", "inf", "nan", "rounded7", "constant"])
def test_free_energies_of_any_origin(dens, probe, fe_case, family):
    """the families of tests/fe_families.py mapped onto Q and R: one draw over both sets, cut in two"""
    Q, R, d2 = fe_case
    both = np.vstack([Q, R])
    pops = expect_pops(block_d2(probe, both, both), [0.2])[0] if family in fe_families.NEEDS_POPS else None
    fe = fe_families.make(family, both, pops, seed=4)
    fe_q, fe_r = fe[:len(Q)].copy(), fe[len(Q):].copy()
    q, r = gpu(Q), gpu(R)
    same_nn(dens.nearest_reference(q, r, gpu(fe_q), gpu(fe_r), pruned=True), expect_nn(d2, fe_q, fe_r), family)
    if family == "nan":
        assert np.isnan(fe_r).any() and info(dens) == (0, 0, 0)   # a NaN in fe_ref: the direct kernel answered
        fe_r = np.where(np.isnan(fe_r), F32(0.5), fe_r).astype(np.float32)
        fe_q[::9] = np.inf
        assert np.isnan(fe_q).any()
        same_nn(dens.nearest_reference(q, r, gpu(fe_q), gpu(fe_r), pruned=True), expect_nn(d2, fe_q, fe_r), "NaN and inf in fe_q")
        assert info(dens)[0] > 0
    if family == "constant":
        # every fe_q at or below the lowest fe_ref: all hd are none while nn stays right
        low = np.full(len(Q), fe_r.min(), dtype=np.float32)
        low[::2] = np.nextafter(fe_r.min(), F32(-np.inf))
        exp = expect_nn(d2, low, fe_r)
        assert (exp[2] == len(R) + 1).all()
        same_nn(dens.nearest_reference(q, r, gpu(low), gpu(fe_r), pruned=True), exp, "all hd none")
        print("all hd none: nn_tiles, nn_mfma, shares", info(dens), "of", tiles(len(Q)) * tiles(len(R)))


# ---- 5 --------------------------------------------------------------------------------------------------------------
def test_a_lower_frame_only_far_away(dens, probe):
    Q, R, fe_q, fe_r, special = cn.far_lower()
    d2 = block_d2(probe, Q, R)
    exp = expect_nn(d2, fe_q, fe_r)
    assert (exp[2][:40] == special).all()
    same_nn(dens.nearest_reference(gpu(Q), gpu(R), gpu(fe_q), gpu(fe_r), pruned=True), exp, "far lower")
    print("far lower: nn_tiles, nn_mfma, shares", info(dens), "of", tiles(len(Q)) * tiles(len(R)))


# ---- 6 --------------------------------------------------------------------------------------------------------------
def test_identities(dens, probe, oracle):
    n, D = 5000, 10
    c = gaussian_blobs(n, D, seed=6)
    rng = np.random.default_rng(6)
    c[rng.integers(0, n, n // 8)] = c[rng.integers(0, n, n // 8)]
    t = gpu(c)
    nn_i, nn_d, _, _ = dens.nearest_reference(t, t, pruned=True)
    first = {}
    for j, row in enumerate(map(bytes, c)):
        first.setdefault(row, j)
    want = np.array([first[bytes(row)] for row in c])
    assert (host(nn_i) == want).all() and (host(nn_d) == 0).all()
    fe = rng.normal(size=n).astype(np.float32)
    S = np.sort(rng.choice(n, 1500, replace=False))
    _, _, hd_i, hd_d = oracle.nearest_neighbors(c, fe)
    got = dens.nearest_reference(gpu(c[S]), t, gpu(fe[S]), gpu(fe), pruned=True)
    assert (host(got[2]).astype(np.int64) == hd_i[S].astype(np.int64)).all()
    assert (host(got[3]).view(np.uint32) == hd_d[S].view(np.uint32)).all()


# ---- 7 --------------------------------------------------------------------------------------------------------------
def rand_fe(Q, R, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, len(Q)).astype(np.float32), rng.uniform(0, 1, len(R)).astype(np.float32)


@pytest.mark.parametrize("D", [3, 10, 30])
def test_scale_edges(dens, probe, D):
    rng = np.random.default_rng(D)
    R = (rng.normal(size=(1500, D)) * 0.02).astype(np.float32)
    Q = (R[:700] + F32(1e4)).astype(np.float32)
    Q[::7] = R[:700:7] + (rng.normal(size=(100, D)) * 0.01).astype(np.float32)
    check(dens, probe, Q, R, *rand_fe(Q, R, 1), "offset 1e4")
    Q = (rng.normal(size=(500, D)) * 0.02 + 1000.0).astype(np.float32)
    check(dens, probe, Q, R, *rand_fe(Q, R, 2), "far away")
    tiny = (rng.normal(size=(900, D)) * 1e-3).astype(np.float32)
    large = (rng.normal(size=(800, D)) * 50.0).astype(np.float32)
    large[::5] = tiny[:160] * F32(3.0)
    check(dens, probe, large, tiny, *rand_fe(large, tiny, 3), "tiny reference")
    check(dens, probe, tiny, large, *rand_fe(tiny, large, 4), "tiny queries")


def test_degenerate_grids(dens, probe):
    for name, Q, R, _ in cp.degenerate_cases():
        check(dens, probe, Q, R, *rand_fe(Q, R, 9), name)


# ---- 8 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 10])
def test_non_finite_rows_and_empty_sets(dens, probe, D):
    Q, R = sets(D, 700, 900, seed=D)
    clean = (Q.copy(), R.copy())
    fe_q, fe_r = rand_fe(Q, R, D)
    Q[3, 0] = np.inf
    Q[10, D - 1] = np.nan
    R[5, 0] = -np.inf
    R[17, D // 2] = np.nan
    d2 = check(dens, probe, Q, R, fe_q, fe_r, "non-finite")
    assert info(dens) == (0, 0, 0)
    exp = expect_nn(d2, fe_q, fe_r)
    assert (exp[0][[3, 10]] == len(R) + 1).all() and not np.isin(exp[0], [5, 17]).any()
    check(dens, probe, clean[0], clean[1], fe_q, fe_r, "clean, after a flagged call in the same workspace")
    assert info(dens)[0] > 0
    empty = gpu(np.zeros((0, D), np.float32))
    got = dens.nearest_reference(gpu(clean[0]), empty, gpu(fe_q), gpu(fe_r[:0]), pruned=True)
    assert (host(got[0]) == 1).all() and (host(got[2]) == 1).all()
    assert (host(got[1]) == FLT_MAX).all() and (host(got[3]) == FLT_MAX).all()
    assert info(dens) == (0, 0, 0)
    got = dens.nearest_reference(empty, gpu(clean[1]), gpu(fe_q[:0]), gpu(fe_r), pruned=True)
    assert got[0].numel() == 0 and got[3].numel() == 0


# ---- 9 --------------------------------------------------------------------------------------------------------------
CHILD_SHARES = r"""
import os, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from clustering_amd import capi, density as dens
from oracle.oracle import Probe
import test_gpu_cross_nn_pruned as t
from crossref import sets
probe = Probe(capi.CANON_ORDER)
for (n_q, n_r), D in (((700, 3000), 10), ((333, 4097), 3)):
    Q, R = sets(D, n_q, n_r, seed=D + n_q)
    fe_q, fe_r = t.rand_fe(Q, R, D)
    t.check(dens, probe, Q, R, fe_q, fe_r, ("shares", D))
    shares = t.info(dens)[2]
    print("shares", D, shares)
    assert shares > 1, shares
print("ok")
"""


def run_child(code, env, *args):
    env = dict(os.environ, **env)
    env.pop("DC_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-c", code, ROOT, *args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


def test_several_shares():
    """DC_SHARE_FLOOR=8 (read once per process: a fresh child): the reference is dealt to several shares, whose results
    merge through the 64-bit minimum"""
    run_child(CHILD_SHARES, {"DC_SHARE_FLOOR": "8"})


# ---- 10 -------------------------------------------------------------------------------------------------------------
def test_more_than_2_24_references(dens):
    """a reference of more than 2^24 positions goes to the every-pair sweep in the same workspace (the population
    sweep's rule, cross_pruned_takes, kept for both pruned sweeps; this kernel's own queue entries would hold 30 bits).  D = 1, refereed by numpy's float32 (q - r)^2 (equal to the probe's d2 there: the CPU premise test)."""
    import torch
    n_r, n_q = 2 ** 24 + 1, 32
    rng = np.random.default_rng(24)
    R = rng.normal(size=(n_r, 1)).astype(np.float32)
    Q = rng.normal(size=(n_q, 1)).astype(np.float32)
    fe_r = ((np.arange(n_r) % 1024) / 1024.0).astype(np.float32)
    fe_q = np.resize(np.array([0.0, 0.5, 2.0, np.inf, 1.0 / 1024.0], dtype=np.float32), n_q)
    exp = [np.zeros(n_q, np.int64), np.zeros(n_q, np.float32), np.zeros(n_q, np.int64), np.zeros(n_q, np.float32)]
    for i in range(n_q):
        d = (Q[i, 0] - R[:, 0]).astype(np.float32)
        d = (d * d).astype(np.float32)
        j = int(np.argmin(d))
        exp[0][i], exp[1][i] = j, d[j]
        m = fe_r < fe_q[i]
        if m.any():
            dm = np.where(m, d, np.inf)
            j = int(np.argmin(dm))
            exp[2][i], exp[3][i] = j, d[j]
        else:
            exp[2][i], exp[3][i] = n_r + 1, FLT_MAX
    got = dens.nearest_reference(gpu(Q), gpu(R), gpu(fe_q), gpu(fe_r), pruned=True)
    same_nn(got, exp, "2^24 + 1 references")
    assert info(dens) == (0, 0, 0)
    dens._nearest_pruned_workspaces.clear()
    torch.cuda.empty_cache()


# ---- 11 -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_next_call_right(dens, probe):
    import torch
    from clustering_amd import capi
    Q, R = sets(65, 100, 200, seed=1)
    with pytest.raises(RuntimeError):
        dens.nearest_reference(gpu(Q), gpu(R), pruned=True)
    Q, R = sets(10, 300, 700, seed=2)
    q, r = gpu(Q), gpu(R)
    with pytest.raises(ValueError):
        dens.nearest_reference(q, r, variant="mfma", pruned=True)
    with pytest.raises(RuntimeError):
        dens.nearest_reference(q, r, variant="cross_pruned")
    need = capi.lib.dc_hip_nearest_cross_pruned_workspace_bytes(300, 700, 10)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(300, dtype=torch.int32, device="cuda")
    d2o = torch.zeros(300, dtype=torch.float32, device="cuda")
    vp = ctypes.c_void_p
    args = (vp(q.data_ptr()), 300, vp(r.data_ptr()), 700, 10, None, None, 0, 300, vp(idx.data_ptr()), vp(d2o.data_ptr()),
            None, None, vp(ws.data_ptr()))
    stream = vp(torch.cuda.current_stream().cuda_stream)
    assert capi.lib.dc_hip_nearest_neighbors_cross_pruned_dev(*args, need - 1, stream) == -5
    assert capi.lib.dc_hip_nearest_neighbors_cross_pruned_dev(*args, need, stream) == 0
    same_nn((idx, d2o), expect_nn(block_d2(probe, Q, R)), "exact workspace")
    check(dens, probe, Q, R, *rand_fe(Q, R, 11), "after the refusals")


# ---- 12 -------------------------------------------------------------------------------------------------------------
def test_assign_frames(dens):
    c = gaussian_blobs(7000, 10, seed=8)
    q, r = gpu(c[:2000]), gpu(c[2000:])
    states = (np.arange(5000) % 7 + 1).astype(np.int32)
    want = dens.assign_frames(q, r, 0.2, states, variant="direct")
    for kw in (dict(pruned_neighbours=True), dict(pruned_neighbours=True, variant="cross_pruned")):
        got = dens.assign_frames(q, r, 0.2, states, **kw)
        for k in want:
            a, b = want[k], got[k]
            if isinstance(a, int):
                assert a == b, (k, kw)
            else:
                assert (host(a).view(np.uint32) == host(b).view(np.uint32)).all(), (k, kw)


# ---- 13 -------------------------------------------------------------------------------------------------------------
CHILD_ORDER = r"""
import os, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from clustering_amd import capi, density as dens
from oracle.oracle import Probe
import test_gpu_cross_nn_pruned as t
assert capi.lib.dc_hip_canon_order().decode() == sys.argv[2] == capi.CANON_ORDER
t.tie_programme(dens, Probe(capi.CANON_ORDER), 10)
print("ok")
"""


@pytest.mark.parametrize("order", ["avx", "fma"])
def test_other_order_libraries(order):
    """the tie cases at D = 10 on the library of another summation order, in a fresh child process"""
    if not os.path.exists(os.path.join(ROOT, "clustering_amd", "lib_" + order, "libdcdensity.so")):
        pytest.fail(f"clustering_amd/lib_{order}/libdcdensity.so is missing: __graft_entry__.build() makes it")
    run_child(CHILD_ORDER, {"DC_CANON_ORDER": order}, order)
